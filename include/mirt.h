/*
 * mirt.h -- C ABI of libmirt.so: the MI355X-native device runtime behind the host
 * interface of eaymerich/2015-RayTracing's Assign10 path tracer.
 *
 * The reference host (Assign10-Path_Tracing/code.js, "A10 code.js" below) talks to its
 * device through the WebCL 1.0 object model (webcl -> context -> queue / program ->
 * kernel / buffer).  Each entry point here is what that binding needs underneath; the
 * comment on each cites the reference call it replaces.  Signatures are plain C
 * (opaque handles, pointers, sizes); no C++ exception crosses this boundary.
 *
 * Conventions
 *   - return 0 (MIRT_OK) or a negative mirt_status; text via mirt_last_error().
 *   - host pointers are borrowed for the duration of the call only: reads/writes of
 *     pageable memory complete before the call returns, whatever `blocking` says (the
 *     reference passes blocking=false and keeps its typed arrays alive until finish()).
 *   - one in-order HIP stream per context (A10 code.js:592 createCommandQueue()).
 *   - handles are reference-free: release exactly once; using a released handle -- or a
 *     handle of the wrong kind -- is MIRT_E_HANDLE, not undefined behaviour (every handle is
 *     validated against a live table keyed by address AND kind).
 *   - a context owns what was created on it: mirt_ctx_destroy releases the buffers, kernels
 *     and graphs the host left behind (the reference host never releases its bouncePaths
 *     kernel, A10 code.js:1444-1455); those handles are MIRT_E_HANDLE afterwards.
 *   - single host thread per context (the reference is a single JS thread).
 */
#ifndef MIRT_H
#define MIRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define MIRT_API __attribute__((visibility("default")))
#else
#define MIRT_API
#endif

typedef struct mirt_ctx mirt_ctx;
typedef struct mirt_buf mirt_buf;
typedef struct mirt_kernel mirt_kernel;

typedef enum mirt_status {
    MIRT_OK = 0,
    MIRT_E_ARG = -1,        /* bad argument (null, size mismatch, index out of range)        */
    MIRT_E_HANDLE = -2,     /* unknown or already released handle                            */
    MIRT_E_NAME = -3,       /* no kernel of that name (WebCL: INVALID_KERNEL_NAME)           */
    MIRT_E_UNSET = -4,      /* enqueue with an argument never set (INVALID_KERNEL_ARGS)      */
    MIRT_E_RANGE = -5,      /* buffer too small for what the launch would touch              */
    MIRT_E_DEVICE = -6,     /* HIP runtime error (message has the hipError string)           */
    MIRT_E_NODEVICE = -7,   /* no gfx950 device / extension not usable                       */
    MIRT_E_DATA = -8        /* device data failed validation (cell offsets not monotone ...) */
} mirt_status;

/* WebCL memory flags (A10 code.js:1083, 1175, 1312: MEM_READ_WRITE / MEM_READ_ONLY / MEM_WRITE_ONLY) */
#define MIRT_MEM_READ_WRITE 1u
#define MIRT_MEM_WRITE_ONLY 2u
#define MIRT_MEM_READ_ONLY 4u

/* ---- platform / device: webcl.getPlatforms(), platform.getDevices(), device.getInfo()
 *      (A10 code.js:483-498, 623-631) ------------------------------------------------- */
MIRT_API int mirt_device_count(void);
MIRT_API int mirt_device_name(int device, char* out, size_t cap);
MIRT_API const char* mirt_version(void);
/* Bumped whenever an existing entry point changes its parameters or the meaning of a value (a caller built against an older header would link and
 * pass shifted arguments).  4: mirt_gather takes n_tiles and a transport enum (round 3); mirt_pass_desc.acu may be NULL (round 4).  Check
 * mirt_abi_version() == MIRT_ABI_VERSION before anything else. */
#define MIRT_ABI_VERSION 4
MIRT_API int mirt_abi_version(void);

/* ---- context + command queue: webcl.createContext(device) + ctx.createCommandQueue()
 *      (A10 code.js:582, 592); release() of both (code.js:1539-1552) ------------------- */
MIRT_API int mirt_ctx_create(int device, mirt_ctx** out);
MIRT_API int mirt_ctx_destroy(mirt_ctx* ctx);
/* last error text of `ctx` (or of the calling thread when ctx is NULL); never NULL */
MIRT_API const char* mirt_last_error(mirt_ctx* ctx);
/* run on a caller-owned hipStream_t (e.g. torch's current stream) instead of the context's own */
MIRT_API int mirt_ctx_set_stream(mirt_ctx* ctx, void* hip_stream);
/* queue.finish() (A10 code.js:1096, 1406, 1533) */
MIRT_API int mirt_finish(mirt_ctx* ctx);

/* ---- buffers: ctx.createBuffer(flags, bytes) (A10 code.js:1083, 1117-1118, 1149, 1175-1177,
 *      1221-1224, 1268-1270, 1312, 1375, 1428), buffer.release() ----------------------- */
MIRT_API int mirt_buf_create(mirt_ctx* ctx, size_t bytes, unsigned flags, mirt_buf** out);
/* adopt device memory owned by the caller (a torch tensor's data_ptr); release() does not free it.  The runtime cannot see writes
 * made to such memory behind its back, so nothing derived from its contents is cached: cell-offset tables are re-validated and
 * triangles re-prepared on every launch that uses a wrapped buffer as geometry. */
MIRT_API int mirt_buf_wrap(mirt_ctx* ctx, void* device_ptr, size_t bytes, mirt_buf** out);
/* tell the runtime that a buffer's contents were changed outside mirt_buf_write / the kernels (through mirt_buf_device_ptr, or by
 * another stream): drops the cached validation / preparation of that buffer and invalidates recordings that relied on it */
MIRT_API int mirt_buf_invalidate(mirt_buf* buf);
MIRT_API int mirt_buf_release(mirt_buf* buf);
MIRT_API size_t mirt_buf_size(const mirt_buf* buf);
MIRT_API void* mirt_buf_device_ptr(const mirt_buf* buf);
/* queue.enqueueWriteBuffer(buf, blocking, offset, nbytes, typedArray, []) (A10 code.js:1153, 1183-1185, ...) */
MIRT_API int mirt_buf_write(mirt_buf* buf, size_t offset, size_t nbytes, const void* host, int blocking);
/* queue.enqueueReadBuffer(buf, blocking, offset, nbytes, typedArray, []) (A10 code.js:1070, 1532) */
MIRT_API int mirt_buf_read(mirt_buf* buf, size_t offset, size_t nbytes, void* host, int blocking);

/* ---- program + kernels: ctx.createProgram(src); program.build(); program.createKernel(name)
 *      (A10 code.js:596-607, 1048, 1087, 1107, 1158, 1206, 1256, 1307, 1348, 1366, 1422, 1446,
 *      1463, 1483).  There is no JIT: `mirt_program_check` scans the OpenCL C text the host
 *      would have compiled and reports, for every `__kernel void NAME(`, whether a built-in
 *      HIP kernel of that name exists; `missing` receives a comma-separated list of those
 *      that do not (the WebCL build log).  Returns the number of missing kernels, or <0. ---- */
MIRT_API int mirt_program_check(mirt_ctx* ctx, const char* source, char* missing, size_t cap);
/* Which assignment's kernel set an OpenCL C text asks for: 10 (Assign10), 7, 4, 1, or 0 = not built (A02/03/05/06/08/09).
 * The kernel NAMES collide across assignments (initTrace, meshTrace), so the sets other than A10's are reached through
 * mirt_kernel_get with a dialect prefix: "A07:meshTrace", "A04:initTrace", "A01:raytrace", ... */
MIRT_API int mirt_program_dialect(const char* source);
/* names: sizeofRay sizeofPoi initAcu initTrace sphereTrace triangleTrace meshTrace lightRender
 * initShadowTrace sphereShadowTrace triangleShadowTrace sceneRender bouncePaths copyToPixel   (A10, A10 code.cl:440-1386)
 * A07:sizeofRay A07:initTrace A07:meshTrace  (A07 code.cl:307-335, 475-626)   A04:sizeofRay A04:initTrace A04:meshTrace
 * (A04 code.cl:200-215, 262-315)   A01:raytrace (A01 code.cl:116-147) */
MIRT_API int mirt_kernel_get(mirt_ctx* ctx, const char* name, mirt_kernel** out);
MIRT_API int mirt_kernel_release(mirt_kernel* k);
/* number of arguments of the kernel (WebCL kernel.getInfo(KERNEL_NUM_ARGS)) */
MIRT_API int mirt_kernel_num_args(const mirt_kernel* k);
/* kernel.setArg(i, typedArray): scalars are 4 bytes, float16 64 bytes, AABB 32 bytes in the
 * host packing (min,1,max,1) (A10 code.js:610-621, 1089, 1127-1131, ...).  Size must match. */
MIRT_API int mirt_kernel_set_arg(mirt_kernel* k, unsigned index, size_t size, const void* value);
/* kernel.setArg(i, webclBuffer) */
MIRT_API int mirt_kernel_set_arg_buf(mirt_kernel* k, unsigned index, mirt_buf* buf);
/* kernel.getWorkGroupInfo(device, KERNEL_PREFERRED_WORK_GROUP_SIZE_MULTIPLE) (A10 code.js:656): 64 */
MIRT_API int mirt_kernel_preferred_multiple(const mirt_kernel* k);
/* queue.enqueueNDRangeKernel(kernel, dim, null, globalWS, localWS) (A10 code.js:1095, 1302, 1330,
 * 1339, 1343, 1399, 1405, 1414, 1503, 1507, 1511, 1519, 1527).  `local` may be NULL. */
MIRT_API int mirt_enqueue(mirt_ctx* ctx, mirt_kernel* k, unsigned dim, const size_t* global, const size_t* local);

/* ---- extension: the whole pass in one launch -------------------------------------------
 * One call == one executeRender() of the reference minus the read-back (A10 code.js:1806-1854):
 * initTrace, closest hits, lightRender, per-light shadow + shade, `bounces` bounce segments,
 * accumulated into `acu`; optionally followed by copyToPixel.  Results are bit-identical to
 * enqueueing the fourteen kernels one by one.  Rows [row0, row0+nrows) of the image are
 * rendered; seeds/acu/pixel/radiance are tile-local (nrows*width[*rpp] elements), ray ids
 * stay global so a frame does not depend on how it is tiled over GPUs. */
#define MIRT_MAX_LIGHTS 8
#define MIRT_MAX_MESHES 16

/* THE CELL TABLE.  cell_offsets is off = uint[n^3 + 1]: cell c (c = (z * n + y) * n + x) holds the slots [off[c], off[c + 1]) of the
 * primitive arrays, and its primitives are tested in slot order, exactly as the reference's kernels read the table.  A table is VALID when
 *   - it is non-decreasing (off[c] <= off[c + 1] for every cell; otherwise MIRT_E_DATA),
 *   - with n > 1, no cell holds 2^24 slots or more (MIRT_E_RANGE), and
 *   - prims (and normals, matid where the set has them) hold at least off[n^3] records (MIRT_E_RANGE).
 * Nothing else is asked of it: off[0] need not be 0, cells may be empty, a primitive may sit in any cell, in several or in none, in any
 * order and more than once, whether its box touches the cell or not.  The result of every entry point is what the reference's kernels
 * compute FOR THAT TABLE -- a primitive missing from a cell it crosses is missed there, as in the reference.
 * The slots before off[0] and the records behind slot off[n^3] belong to no cell: they never influence a result, whatever they hold (a
 * non-finite record there can only cost time: the optimistic kernel may hand work to the exact one).  The tables of mirt_grid_build and of
 * the reference's split*Data are the special case off[0] == 0, no slack, input order. */
typedef struct mirt_grid {          /* one cell-sorted primitive set as the host uploads it        */
    mirt_buf* prims;                /* spheres: float4 (c, r^2) | triangles: 3 x float4 positions  */
    mirt_buf* normals;              /* triangles: 3 x float4 normals; NULL for spheres             */
    mirt_buf* matid;                /* uint per primitive; NULL for a mesh (uses mesh_matid)       */
    mirt_buf* cell_offsets;         /* uint[n^3 + 1]: any valid table (THE CELL TABLE, above)      */
    float bounds[8];                /* (min,1,max,1), bounds2AABB, A10 code.js:610-621             */
    uint32_t n_slabs;
    uint32_t mesh_matid;
} mirt_grid;

typedef struct mirt_light {         /* Light.to{Shadow,SceneRender,LightRender}Info, A10 code.js:323-352 */
    float shadow[16];
    float scene[16];
    float light[16];
} mirt_light;

typedef struct mirt_pass_desc {
    uint32_t struct_size;           /* sizeof(mirt_pass_desc), for ABI evolution                   */
    uint32_t width, height, rays_per_pixel;
    uint32_t row0, nrows;           /* row tile; nrows == 0 means the whole image.  A tile holds at most 2^32 - 256 rays
                                     * (nrows * width * rays_per_pixel: MIRT_E_ARG beyond; cut the rows over more calls) */
    uint32_t bounces;               /* 5 == reference (A10 code.js:1829)                           */
    uint32_t pass_index;            /* 1-based `passes` counter (A10 code.js:1850)                 */
    float cam[16];                  /* Camera.toFloat32Array, A10 code.js:250-258                  */
    float scene_bounds[8];
    float focal_length, lens_rad;   /* A10 code.js:1129-1130 (lens_rad = lens_diameter/2)          */
    uint32_t n_lights, n_meshes;
    const mirt_grid* spheres;       /* NULL: none                                                  */
    const mirt_grid* triangles;     /* NULL: none                                                  */
    const mirt_grid* meshes;        /* [n_meshes]                                                  */
    const mirt_light* lights;       /* [n_lights]                                                  */
    mirt_buf* material;             /* float4 per material (splitMaterialData, code.js:1774-1782)  */
    mirt_buf* seeds;                /* int32 per local ray, read-modify-write                      */
    mirt_buf* acu;                  /* float4 per local ray, accumulated into (zero it first).  May be NULL for a frame's first pass
                                     * (mirt_render_first_pass) that resolves its pixels itself: see below                       */
    mirt_buf* pixel;                /* optional: uchar4 per local pixel, written by copyToPixel    */
    mirt_buf* radiance;             /* optional: float4 per local pixel, un-scaled sequential sums */
} mirt_pass_desc;

/* rays_per_pixel must be k*k, as the reference host makes it (A10 code.js:540): MIRT_E_ARG otherwise */
MIRT_API int mirt_render_pass(mirt_ctx* ctx, const mirt_pass_desc* desc);
/* The first pass of a frame with preRender's initAcu (A10 code.js:1078-1099, code.cl:448-456) folded in: `acu` is not read, every
 * accumulator starts at (0,0,0,0).  Saves the zeroing launch and half of the pass's memory traffic; results equal
 * mirt_zero(acu) + mirt_render_pass.
 * copyToPixel INSIDE the pass: when a pixel or radiance buffer is given and rays_per_pixel divides 256 (1, 4, 16, 64, 256: a block of
 * 256 consecutive ray ids then holds whole pixels), every block sums its pixels' accumulators in LDS in copyToPixel's order (A10
 * code.cl:1366-1386: sequential in i, from +0) and writes pixel / radiance itself -- no second kernel, no re-read of the accumulators.
 * Then, and only then, `acu` may be NULL: nothing per ray but the seed touches memory (8 B per sample + 20 B per pixel) and the
 * 16 bytes per ray are never allocated; with `acu` given it is written as before (what a second progressive pass needs).  Results
 * are bit-identical either way.  In this mode the optimistic / exact kernel pair hands over whole blocks of 256 samples
 * (mirt_pass_deferred counts them as such).  MIRT_INPASS_RESOLVE=0 in the environment keeps the separate copyToPixel.
 * A LATER pass (mirt_render_pass) with a pixel or radiance buffer resolves inside the pass under the same condition -- `acu` is then read and
 * written as ever, and the separate copyToPixel's second read of it is saved; the runtime's command-stream fusion (mirt_ctx_set_fusion) folds the
 * host's recorded copyToPixel into the pass the same way, with the factor the host passed.
 * MORE than 256 rays per pixel, any count (17 x 17 = 289, BASELINE config 5's 32 x 32 = 1024, ...): the pixel's rays are cut, in ray order,
 * into power-of-two segments of at most 256 -- floor(rays_per_pixel / 256) of 256, then one per set bit of the rest, largest first (289: 256,
 * 32, 1) -- and the pass is queued as one launch per segment, each rendering that segment of every pixel (a block holds 256 / length pixels'
 * segments) and going on from the sums the launch before it left in `radiance` (or in the context's scratch buffer when the caller passes
 * none): the reference's one chain of additions, cut at segment boundaries and carried through memory at 16 B per pixel and launch instead of
 * 16 B per ray.  A first pass may leave `acu` NULL at every such count; results are bit-identical.  With `acu` given, a pass resolves inside
 * the kernel only at 256 times a power of two up to 32 (1024, 4096); at the other counts above 256 it writes `acu` and runs the separate
 * copyToPixel. */
MIRT_API int mirt_render_first_pass(mirt_ctx* ctx, const mirt_pass_desc* desc);
/* Several progressive passes in ONE call (A10 code.js:1806-1853: executeRender, executeCopyToPixel, passes++ -- n_passes times).  Results equal,
 * bit for bit in every buffer the caller passes (seeds, acu if given, pixel, radiance), this sequence:
 *   mirt_render_first_pass (flags & MIRT_PASSES_FRESH) or mirt_render_pass, at desc->pass_index;
 *   then mirt_render_pass at pass_index + 1 .. pass_index + n_passes - 1.
 * Pixel and radiance are those of the last pass (MIRT_PASSES_EVERY_FRAME: of every pass, below) (tone factor 1 / (rays_per_pixel * (pass_index + n_passes - 1))).  Passes interact only through a
 * ray's own seed and its own accumulator, so one launch runs every sample through all n_passes passes, the accumulator on chip, and writes the
 * seeds (and `acu`) once: a multi-pass frame needs no per-ray accumulator and moves none between the passes.
 * `acu` may be NULL exactly where a first pass may do without it: MIRT_PASSES_FRESH, a pixel or radiance buffer, rays_per_pixel dividing 256 or
 * above 256 (and MIRT_INPASS_RESOLVE not 0) -- except rays_per_pixel 1, whose rows are coupled through seeds[col] (A10
 * code.cl:429): the call then queues n_passes ordinary passes and needs `acu`.  NULL elsewhere is MIRT_E_ARG.  n_passes is 1..64 (one launch lasts
 * about n_passes single passes); row tiles and global ray ids work as in mirt_render_pass.  mirt_pass_deferred counts the samples (blocks) handed
 * to the exact kernel in the same unit as for one pass -- such a sample re-runs all of its passes; mirt_pass_timing covers the whole call.
 * Not while capturing (MIRT_E_ARG). */
#define MIRT_PASSES_FRESH 1u            /* the batch starts the frame: acu starts at zero and is not read */
/* A frame after EVERY pass (A10 code.js:1806-1854 shows one after each executeRender): `pixel` then holds n_passes RGBA8 frames back to back, frame p at
 * byte p * npix * 4, and `radiance` n_passes float4 frames, frame p at byte p * npix * 16 (npix: the tile's pixels).  Either may be NULL, not both.  Frame p
 * equals, bit for bit, pixel / radiance after the (p+1)-th call of the ordinary sequence above, tone factor 1 / (rays_per_pixel * (pass_index + p));
 * seeds and acu end as without the flag.  Where the passes resolve in the kernel (see mirt_render_first_pass: rays_per_pixel > 1 dividing 256 or above
 * 256, fresh and acu-free, or with acu at the counts that resolve beside it) every frame comes from the same launch(es), the sums of a pixel of more than
 * 256 rays alternating between two carry arrays of n_passes frames (the caller's radiance and context scratch); elsewhere the call queues n_passes
 * ordinary passes, each writing its frame slot.  A buffer smaller than n_passes frames is MIRT_E_ARG and nothing runs.  A library without the flag
 * answers it with MIRT_E_ARG (unknown flags): that is how a host detects it. */
#define MIRT_PASSES_EVERY_FRAME 2u
#define MIRT_MAX_PASSES_PER_CALL 64u
MIRT_API int mirt_render_passes(mirt_ctx* ctx, const mirt_pass_desc* desc, uint32_t n_passes, uint32_t flags);
/* First-hit GUIDE BUFFERS of the row tile, for a denoiser or a-trous filter behind a few-rays-per-pixel frame.  Per tile-local pixel, over its
 * rays pixel * rays_per_pixel + i in sample order i = 0 .. rays_per_pixel - 1 (copyToPixel's order, A10 code.cl:1377-1380), each ray as initTrace
 * and the closest-hit stage (sphereTrace, triangleTrace, every meshTrace in upload order) leave it, before lightRender and any shading:
 *   normal_hits [pixel] = float4(sum Poi.normal.x, sum .y, sum .z, number of hit samples)
 *   albedo_depth[pixel] = float4(sum material[matId].x, sum .y, sum .z, sum Ray.maxt)
 * sequential fp32 sums from +0 over the HIT samples only, un-normalised like `radiance`; a pixel without a hit is all +0 in both.  A sample is a
 * hit when the stage leaves a live vertex -- Poi.matId >= 0, the reference's own test (initTrace resets it to -1, code.cl:538-541; sceneRender
 * shades iff matId >= 0, code.cl:1336); an id past the material table is not a hit and reads nothing.  The guides describe SURFACES: an emitter in
 * front of the surface (lightRender) is not considered.  Poi.normal and Ray.maxt are the bits the kernel-by-kernel path stores.
 * Reads of the descriptor: the image size, rays_per_pixel, row0 / nrows, cam, scene_bounds, focal_length, lens_rad, the primitive sets and
 * material.  Ignored, and free to be NULL or 0: seeds, acu, pixel, radiance, the lights, bounces, pass_index.  Either output may be NULL, not both
 * (MIRT_E_ARG).  Checks as in mirt_render_pass (descriptor size, tile inside the image, k x k rays: MIRT_E_ARG; cell tables: MIRT_E_DATA; a
 * buffer too small: MIRT_E_RANGE); when one fails nothing is written.  Nothing but the two outputs is ever written: the k x k lens grid draws
 * nothing from the seeds, so the guides are the same for every pass of a frame.  rays_per_pixel == 1 draws its lens sample from seeds[col]
 * (code.cl:429) and is refused (MIRT_E_ARG).  Ray ids are global: a tile's guides equal the same rows of the whole frame's.  Not while capturing
 * (MIRT_E_ARG).  MIRT_ABI_VERSION is unchanged: a host detects the entry point by its symbol. */
MIRT_API int mirt_render_guides(mirt_ctx* ctx, const mirt_pass_desc* desc, mirt_buf* normal_hits, mirt_buf* albedo_depth);
/* A frame's FIRST PASS AND ITS GUIDES in one call.  Every buffer the caller passes -- seeds, acu if given, pixel, radiance, normal_hits,
 * albedo_depth -- ends bit for bit as after mirt_render_first_pass(ctx, desc) followed by mirt_render_guides(ctx, desc, normal_hits,
 * albedo_depth): the guides are the values the pass itself holds right after its primary rays' closest-hit stage, before lightRender, and
 * mirt_render_guides re-creates every primary ray and repeats that search only to arrive at them.  `desc` is the pass's descriptor, unchanged.
 * Checks: those of both calls, all before anything is queued -- when one fails nothing is written at all, neither the guides nor the pass's
 * buffers.  Either guide output may be NULL, not both (MIRT_E_ARG); rays_per_pixel == 1 is MIRT_E_ARG (the guides' own rule); a guide buffer
 * smaller than the tile's pixels x 16 B is MIRT_E_RANGE; a guide buffer whose bytes are, or overlap, those of any buffer of the descriptor or
 * of the other guide is MIRT_E_ARG; not while capturing (MIRT_E_ARG).  A held command stream (mirt_ctx_set_fusion) is flushed first.
 * ROUTE.  The call works at every k x k count above 1; which launches it queues is the library's matter.  ONE LAUNCH (per kernel of the
 * optimistic / exact pair): where the pass resolves its pixels in the kernel (see mirt_render_first_pass) as one segment with rays_per_pixel
 * 4, 16 or 64, a pixel's samples are rays_per_pixel consecutive lanes of one wave, and the pass's kernel adds their eight values in sample
 * order and writes the guides itself.  EVERYWHERE ELSE -- 256 rays (a pixel spans four waves), counts that do not divide 256 or are above it,
 * MIRT_INPASS_RESOLVE=0, acu given with neither pixel nor radiance -- the call queues the pass and then the guide launches exactly as the two
 * calls would.  MIRT_GUIDED_PASS=0 in the environment forces that everywhere (an A/B switch).  mirt_ctx_guided_passes: how many calls of this
 * context took the one-launch route (this call's and mirt_render_passes_guided's).  What the call does not do: several passes in one launch
 * (that is mirt_render_passes_guided), a one-launch route at 256 rays per pixel, guides from a later pass (mirt_render_pass) -- they are the
 * same for every pass of a frame, so the first pass is where they are taken.
 * The optimistic kernel writes a block's guides before it knows whether the block stays inside the guard windows; a block that does not is
 * re-run whole by the exact kernel, which writes the same pixels' guides again, later on the same stream.  The outputs are therefore final
 * when the call's launches have completed (stream order, mirt_finish), like every other output of the pass -- not before.
 * MIRT_ABI_VERSION is unchanged: a host detects the two entry points by their symbols. */
MIRT_API int mirt_render_first_pass_guided(mirt_ctx* ctx, const mirt_pass_desc* desc, mirt_buf* normal_hits, mirt_buf* albedo_depth);
MIRT_API int mirt_ctx_guided_passes(mirt_ctx* ctx, uint64_t* count);
/* SEVERAL PASSES AND THE FRAME'S GUIDES in one call.  Every buffer the caller passes -- seeds, acu if given, pixel, radiance (n_passes frames
 * each with MIRT_PASSES_EVERY_FRAME), normal_hits, albedo_depth -- ends bit for bit as after mirt_render_passes(ctx, desc, n_passes, flags)
 * followed by mirt_render_guides(ctx, desc, normal_hits, albedo_depth), fresh or not and at any pass_index: the k x k lens grid draws nothing from
 * the seeds, so the guides are those of every pass of the frame, and the launch takes them from the first pass it runs.
 * Checks: those of both calls, all before anything is queued -- when one fails nothing is written at all.  n_passes and flags as in
 * mirt_render_passes; either guide output may be NULL, not both (MIRT_E_ARG); rays_per_pixel == 1 is MIRT_E_ARG; a guide buffer smaller than the
 * tile's pixels x 16 B is MIRT_E_RANGE; a guide buffer whose bytes are, or overlap, those of any buffer of the descriptor (pixel and radiance at
 * their whole n_passes frames) or of the other guide is MIRT_E_ARG; not while capturing (MIRT_E_ARG).
 * ROUTE.  ONE LAUNCH (per kernel of the optimistic / exact pair): where mirt_render_passes runs the batch as one launch -- with or without a
 * frame after every pass -- that resolves its pixels in the kernel as one segment with rays_per_pixel 4, 16 or 64, the launch's first pass adds a
 * pixel's eight values lane by lane right after its primary rays' closest-hit stage and writes the guides itself; mirt_ctx_guided_passes counts
 * the call.  EVERYWHERE ELSE -- 256 rays, counts that do not divide 256 or are above it, acu given with neither pixel nor radiance,
 * MIRT_INPASS_RESOLVE=0, MIRT_GUIDED_PASS=0, several passes with MIRT_MULTIPASS_REUSE forcing the pairing that is not the default one (the guided
 * multi-pass kernels are built for the default; one pass has no pairing), several passes of a scene with a grid of more than one cell (measured: writing the guides from the grid kernels'
 * multi-pass loop was slower than the guide launches behind it), n_passes ordinary passes (MIRT_PASSES_EVERY_FRAME where the passes do not resolve in the kernel, or with n_passes
 * 1) -- the call queues what mirt_render_passes queues and then the guide launches, exactly as the two calls would.  With n_passes 1 and no
 * MIRT_PASSES_EVERY_FRAME the call is mirt_render_first_pass_guided (MIRT_PASSES_FRESH) in every buffer.
 * As there, an optimistic block writes its guides before its verdict, which may come in any pass; the exact kernel re-runs such a block from
 * its first pass and writes the same pixels' guides again, so the outputs are final when the call's launches have completed.  mirt_pass_deferred
 * and mirt_pass_timing mean what they mean for mirt_render_passes.  What the call does not do: a one-launch route at 256 rays per pixel or
 * above, graph capture.  MIRT_ABI_VERSION is unchanged: a host detects the entry point by its symbol. */
MIRT_API int mirt_render_passes_guided(mirt_ctx* ctx, const mirt_pass_desc* desc, uint32_t n_passes, uint32_t flags, mirt_buf* normal_hits,
                                       mirt_buf* albedo_depth);
/* RAY QUERIES: the closest hit, or whether anything is hit at all, for `count` rays the CALLER supplies -- picking, autofocus, visibility between
 * two points, ambient occlusion, baking.  rays[i] is a mirt_ray, used as given: d is not normalised, so t is in units of |d|, as the kernels
 * treat Ray.d.  `scene` is a pass descriptor of which only struct_size and the primitive sets (spheres, triangles, meshes, n_meshes) are read;
 * the image size, rays_per_pixel, tile, camera, lens, lights, material, seeds, acu, pixel, radiance, bounces and pass_index are ignored and free
 * to be 0 or NULL.
 * CLOSEST.  hits[i] is defined, bit for bit in every field, as what the kernel-by-kernel path leaves in Ray.maxt and Poi when
 * Ray{o, d, mint, maxt} and a Poi reset as initTrace resets it (A10 code.cl:538-541: p = 0, normal = 0, matId = -1) run through sphereTrace,
 * triangleTrace and every meshTrace in upload order (code.js:1809-1813): t is the final Ray.maxt; normal, p and mat_id are the final Poi.  A miss
 * is (0, 0, 0, the input maxt, 0, 0, 0, -1); a dead ray (mint == maxt) is a miss.  mat_id is reported raw: no material is read, an id past the
 * material table is the caller's to judge.  sets[i] (optional, uint32) is the index, in that stage order, of the set whose primitive won, or
 * 0xFFFFFFFF: index 0 is the spheres when present, then the loose triangles, then the meshes.  The primitive's slot is not reported (in a grid a
 * primitive has one slot per cell it touches, and which one wins is the walk's matter).  hits or sets may be NULL, not both.
 * OCCLUDED.  occluded[i] (uint8) is sceneRender's own test (code.cl:1350): 1 iff mint == maxt after sphereShadowTrace, triangleShadowTrace and a
 * triangleShadowTrace per mesh in upload order have run on the ray.  A ray that enters dead is therefore reported 1.  No t is delivered.
 * CHECKS, all before anything is queued; nothing is written when one fails.  MIRT_E_ARG: a NULL descriptor or a wrong struct_size, count above
 * 2^32 - 256, hits and sets both NULL (occluded NULL), an output whose bytes meet the rays', a geometry buffer's or the other output's, a call
 * while capturing.  MIRT_E_RANGE: a buffer shorter than count records.  MIRT_E_DATA: a cell table that fails validation.  MIRT_E_HANDLE: a bad
 * context or buffer.  count == 0 is MIRT_OK and queues nothing.  A held command stream (mirt_ctx_set_fusion, frame fusion) is flushed first;
 * wrapped geometry is re-validated as for a pass.
 * KERNELS.  One launch, one lane per ray (csrc/pt_kernels_rays.hip) -- by default the optimistic / exact pair PER RAY: a ray the ray-side guard
 * refuses (mirt_debug_numerics op 28: every |d_k| in [2^-40, 2^40], every o_k zero or |o_k| in [2^-30, 2^20]) or whose grid walk defers is redone
 * by the exact kernel; mirt_ctx_set_exact_only is honoured.  A caller's rays need not be coherent, and an axis-parallel direction (a zero
 * component of d) is outside the guard: such batches run mostly in the exact kernel, with the same results.  mirt_trace_deferred: how many rays
 * the last trace call re-ran in the exact kernel, counted when asked, like mirt_pass_deferred.  Rays are independent: a caller with N devices
 * splits its batch.  MIRT_ABI_VERSION is unchanged: a host detects the entry points by their symbols. */
typedef struct mirt_ray { float o[3]; float mint; float d[3]; float maxt; } mirt_ray;          /* 32 bytes */
typedef struct mirt_hit { float normal[3]; float t; float p[3]; int32_t mat_id; } mirt_hit;   /* 32 bytes */
MIRT_API int mirt_trace_closest(mirt_ctx* ctx, const mirt_pass_desc* scene, mirt_buf* rays, uint64_t count, mirt_buf* hits, mirt_buf* sets);
MIRT_API int mirt_trace_occluded(mirt_ctx* ctx, const mirt_pass_desc* scene, mirt_buf* rays, uint64_t count, mirt_buf* occluded);
MIRT_API int mirt_trace_deferred(mirt_ctx* ctx, uint64_t* rays);
/* PATH RADIANCE OF CALLER-SUPPLIED RAYS: what the path tracer computes along `count` rays of the caller's own -- a panoramic, fisheye or
 * orthographic camera, a light probe, a light-map texel, the continuation of a path whose first hit came from a rasteriser.  It is
 * executeRender (A10 code.js:1806-1854) without initTrace and copyToPixel, in one launch.
 * BUFFERS.  rays[i] is a mirt_ray, 32 bytes, used as given: d is not normalised.  seeds[i] is an int32, read and written.  radiance[i] is a
 * float4, the ray's ACCUMULATOR exactly as the kernel-by-kernel path's acu[i] ends: rgb are sums, w is the number of contributions; dividing is
 * the caller's.  Of `scene` are read: struct_size, the primitive sets (spheres, triangles, meshes, n_meshes), lights / n_lights, material and
 * bounces; everything else -- image size, rays_per_pixel, tile, camera, lens, seeds, acu, pixel, radiance, pass_index -- is ignored and free to
 * be 0 or NULL.
 * DEFINITION, bit for bit in every field.  Ray i runs rd->samples times, j = 0 .. samples - 1, its seed and its accumulator carried from one
 * sample to the next; the accumulator starts at (0, 0, 0, 0), initAcu (code.cl:448-456), or with MIRT_RADIANCE_ACCUMULATE at radiance[i] as
 * given.  Each sample is what the kernel-by-kernel path leaves in acu[i] and seeds[i] when
 *   1. the Ray buffer entry is the caller's {o, d, mint, maxt};
 *   2. the Poi is reset as initTrace resets it (code.cl:538-541): matId = -1, atte = (1, 1, 1);
 *   3. sphereTrace, triangleTrace and every meshTrace run in upload order (code.js:1809-1813);
 *   4. lightRender runs once per light (code.cl:600-629) -- unless MIRT_RADIANCE_NO_EMITTERS is set: the ray continues a path whose vertex
 *      already sampled the lights, so an emitter it meets adds nothing and does not end it;
 *   5. per light: initShadowTrace, then sphereShadowTrace, triangleShadowTrace and a triangleShadowTrace per mesh, then sceneRender
 *      (code.js:1817-1826);
 *   6. `bounces` times: bouncePaths, then the closest-hit kernels of step 3, then the per-light block of step 5 (code.js:1829-1846)
 * have run.  CONSEQUENCES.  A ray that enters dead (mint == maxt) or misses everything adds nothing and draws nothing: its seed is unchanged
 * and its radiance is (0, 0, 0, 0), or its previous value with MIRT_RADIANCE_ACCUMULATE.  A material id past the table shades nothing, as in the
 * pass.  One call with samples = a + b equals a call with a followed by a call with b and MIRT_RADIANCE_ACCUMULATE.  The camera's own rays, as
 * initTrace stores them at a k x k count above 1, run with the pass's seeds, samples = 1 and the pass's bounces, give a pass: radiance equals the
 * acu a fresh mirt_render_first_pass writes, and the seeds end equal to the pass's.
 * CHECKS, all before anything is queued; nothing is written when one fails, and the context works afterwards.  MIRT_E_ARG: a wrong struct_size
 * in either descriptor, samples 0 or above MIRT_RADIANCE_MAX_SAMPLES, unknown flags, reserved != 0, count above 2^32 - 256, NULL seeds or
 * radiance, n_lights above MIRT_MAX_LIGHTS or n_meshes above MIRT_MAX_MESHES, a NULL light or mesh array with a count above 0, seeds or radiance
 * whose bytes meet the rays', each other's, a geometry buffer's or the material's (both are written), a call while capturing.  MIRT_E_RANGE: a
 * buffer shorter than count records, a material table shorter than one entry.  MIRT_E_DATA: a cell table that fails validation.  MIRT_E_HANDLE:
 * a bad context or buffer, the material included.  count == 0 is MIRT_OK and queues nothing.  A held command stream (mirt_ctx_set_fusion, frame
 * fusion) is flushed first; wrapped geometry is re-validated as for a pass.
 * KERNEL.  One launch, one lane per ray walking its samples in order (csrc/pt_kernels_rays.hip k_traceRadiance: the pass's closest-hit loop,
 * lightRender, per-light stage and bounce) -- by default the optimistic / exact pair PER RAY, like the ray queries: a ray whose primary ray, or
 * any shadow or bounce ray of any of its samples, the ray-side guard refuses, or whose grid walk defers, writes neither its seed nor its
 * radiance and is redone from the start, all samples, by the exact kernel; mirt_ctx_set_exact_only is honoured.  mirt_radiance_deferred: the
 * rays the last mirt_trace_radiance re-ran in the exact kernel, counted when asked, like mirt_trace_deferred.  Not built: a per-pixel reduction
 * of the output, tiling over N devices (rays are independent: a caller splits its batch), graph capture, importance other than the pass's own,
 * reuse of the primary ray's hit by the samples after the first.  MIRT_ABI_VERSION is unchanged: a host detects the entry points by their
 * symbols. */
#define MIRT_RADIANCE_ACCUMULATE 1u    /* radiance[i] is read and carried on; without it every accumulator starts at (0,0,0,0), initAcu */
#define MIRT_RADIANCE_NO_EMITTERS 2u   /* lightRender is not run on the caller's ray: the ray continues a path whose vertex already sampled the lights */
#define MIRT_RADIANCE_MAX_SAMPLES 64u
typedef struct mirt_radiance_desc { uint32_t struct_size, samples, flags, reserved; } mirt_radiance_desc;
MIRT_API int mirt_trace_radiance(mirt_ctx* ctx, const mirt_pass_desc* scene, const mirt_radiance_desc* rd, mirt_buf* rays, uint64_t count,
                                 mirt_buf* seeds, mirt_buf* radiance);
MIRT_API int mirt_radiance_deferred(mirt_ctx* ctx, uint64_t* rays);
/* PANORAMIC, FISHEYE AND ORTHOGRAPHIC CAMERAS: a frame of a camera other than the reference's thin lens in ONE launch -- the rays made in
 * registers, traced as mirt_trace_radiance traces them and reduced to pixels inside the block.  By hand it was three launches and three trips
 * through memory per sample (32 B per ray written and read, 16 B per accumulator written and read); here a sample costs its seed, 8 B.
 * THE RAYS, defined once for both calls.  Every operation is ONE fp32 operation rounded on its own, in the order written; nothing is an fma
 * except inside sincos.  `/` is the correctly rounded fp32 quotient, sqrt_cr(x) = (float)sqrt((double)x) the correctly rounded root, sincos the
 * contract's sin and cos (csrc/pt_numerics.hpp cl_sincos): ONE contract, libmirt.so and libmirt_default.so give the same bits.
 *   Global pixel (x, y), y = row0 + tile row; sample i = 0 .. rpp - 1, rpp = k * k, sy = i div k, sx = i mod k.  The tile-local ray id is
 *   ((y - row0) * width + x) * rpp + i; seeds and rays are tile-local, positions use the global y: a tile's rays equal the same rows of the frame's.
 *     fx = (float)x + ((float)sx + 0.5f) * ik, ik = 1 / k (exact: k is a power of two); fy likewise from y and sy
 *     u = fx / (float)width, v = fy / (float)height;   a = (u + u) - 1.0f, b = 1.0f - (v + v)        (row 0 is the top)
 *   ORTHOGRAPHIC   ta = a * half_w, tb = b * half_h;  o.c = (eye.c + right.c * ta) + up.c * tb;  d = forward
 *   EQUIRECT       phi = a * 0x1.921fb6p+1f, th = b * 0x1.921fb6p+0f;  (sp, cp) = sincos(phi), (st, ct) = sincos(th);
 *                  lx = sp * ct, ly = st, lz = cp * ct;  d.c = (right.c * lx + up.c * ly) + forward.c * lz;  o = eye
 *   FISHEYE        r = sqrt_cr(a * a + b * b).  When r <= 1.0f is false the sample is DEAD: o = eye, d = forward, mint = maxt = 0.  Otherwise
 *                  ang = r * half_angle, (sa, ca) = sincos(ang), q = r > 0 ? sa / r : 0;  lx = a * q, ly = b * q, lz = ca;  d and o as EQUIRECT
 *   Every live ray has mint = t_min and maxt = t_max.  No jitter: nothing is drawn from the seeds, like the reference's k x k lens grid.  eye,
 *   right, up and forward are used as given, neither normalised nor orthogonalised.
 * mirt_view_rays writes the tile's width * nrows * rpp mirt_ray records and nothing else.
 * mirt_render_view: everything the caller passes ends, bit for bit, as after (1) mirt_view_rays into a ray buffer, (2) mirt_trace_radiance(ctx,
 * scene, {samples 1, flags 0}, rays, count, seeds, acc) on them -- the same fields of `scene` are read: the sets, lights, material, bounces; a
 * dead sample adds nothing and draws nothing -- (3) per tile pixel p, radiance[p] = the sequential fp32 sum of acc[p * rpp + i], i = 0 .. rpp - 1,
 * all four channels, from +0 or, with MIRT_VIEW_ACCUMULATE, from radiance[p] as given: copyToPixel's order (A10 code.cl:1377-1380), (4) pixel[p] =
 * copyToPixel's own tone map of that sum with m = tone.  The rays and the per-ray accumulators never reach memory.  seeds (int32 per tile ray)
 * are read and written; radiance (float4 per tile pixel) and pixel (RGBA8 per tile pixel) may each be NULL, not both; ACCUMULATE needs radiance.
 * Progressive frames: call p = 1, 2, ... with ACCUMULATE from the second on and tone = 1 / (rpp * p).
 * CHECKS, all before anything is queued; nothing is written when one fails, and the context works afterwards.  MIRT_E_ARG: a wrong struct_size
 * in either descriptor, an unknown model or flag, k not in {1, 2, 4, 8, 16}, width or height 0 or above 65535, a tile outside the image or of
 * more than 2^32 - 256 rays, a non-finite eye or basis component, ORTHOGRAPHIC half_w or half_h not finite or <= 0, FISHEYE half_angle not
 * finite, <= 0 or > pi, t_min negative or not finite, t_max NaN or <= t_min, tone not finite or <= 0 when pixel is given, NULL seeds, both
 * outputs NULL, ACCUMULATE without radiance, outputs whose bytes meet each other's, the seeds', a geometry buffer's or the material's, the light
 * and mesh count rules of mirt_trace_radiance, a call while capturing.  MIRT_E_RANGE: a buffer shorter than the tile's rays or pixels, a material
 * table shorter than one entry.  MIRT_E_DATA: a cell table that fails validation.  MIRT_E_HANDLE: a bad context or buffer.  A held command
 * stream is flushed first; wrapped geometry is re-validated as for a pass.
 * KERNELS (csrc/pt_kernels_rays.hip; a sample's ray is csrc/pt_view.hpp's, the checks and the plan csrc/pt_view_plan.hpp's).  k_viewRays: one
 * lane per ray.  k_viewPass: k_traceRadiance's body with the ray made in registers, then the pass's in-block resolve; a block is 256 consecutive
 * ray ids = 256 / rpp whole pixels.  By default the optimistic / exact pair PER BLOCK: a block with a primary, shadow or bounce ray the ray-side
 * guard refuses, or a walk that defers, writes neither its seeds nor its pixels and is re-run whole by the exact kernel;
 * mirt_ctx_set_exact_only is honoured.  An ORTHOGRAPHIC camera whose `forward` has a zero component is outside the ray-side guard for every ray
 * (|d_k| >= 2^-40): its frames run wholly in the exact kernel, with the same results.  mirt_view_deferred: the rays the last mirt_render_view
 * re-ran in the exact kernel, counted when asked, like mirt_radiance_deferred, in whole blocks of 256.
 * The first-hit guides of these cameras are mirt_view_guides and mirt_render_view_guided, below; what they write is what mirt_filter_atrous reads,
 * so a few-rays-per-pixel panorama is filtered like a thin-lens frame.  Their ambient occlusion is mirt_view_ao, below mirt_render_ao.
 * NOT BUILT: the upsampler for these cameras; jitter
 * or a lens on them; k that is not a power of two, or above 16; more than one sample per ray per call; a multi-device helper (tiles take global positions, so a caller can split the rows); graph capture.
 * MIRT_ABI_VERSION is unchanged: a host detects the entry points by their symbols. */
#define MIRT_VIEW_ORTHOGRAPHIC 0u
#define MIRT_VIEW_EQUIRECT     1u   /* 360 x 180 degrees, longitude along x, latitude along y */
#define MIRT_VIEW_FISHEYE      2u   /* equidistant, the circle inscribed in the image window  */
#define MIRT_VIEW_ACCUMULATE   1u   /* flags: radiance[pixel] is read and the chain of additions goes on from it */
typedef struct mirt_view_desc {
    uint32_t struct_size, model, width, height;   /* the WHOLE image, 1 .. 65535 each                  */
    uint32_t k;                                   /* samples per axis: 1, 2, 4, 8 or 16; rpp = k * k   */
    uint32_t row0, nrows;                         /* row tile as in mirt_pass_desc; nrows 0 = whole    */
    uint32_t flags;
    float eye[3], right[3], up[3], forward[3];    /* used as given: not normalised, not orthogonalised */
    float half_w, half_h;                         /* ORTHOGRAPHIC: half extents of the window, > 0     */
    float half_angle;                             /* FISHEYE: radians at the circle's rim, (0, pi]     */
    float t_min, t_max;                           /* every live ray's mint / maxt; 0 <= t_min < t_max, t_max may be +inf */
    float tone;                                   /* copyToPixel's m; read only when `pixel` is given  */
} mirt_view_desc;
MIRT_API int mirt_view_rays(mirt_ctx* ctx, const mirt_view_desc* view, mirt_buf* rays);
MIRT_API int mirt_render_view(mirt_ctx* ctx, const mirt_pass_desc* scene, const mirt_view_desc* view, mirt_buf* seeds, mirt_buf* radiance, mirt_buf* pixel);
MIRT_API int mirt_view_deferred(mirt_ctx* ctx, uint64_t* rays);
/* BATCHED VIEW CAMERAS: the frames of n_frames cameras in ONE call and one launch (pair) -- a light probe or a data-set view is a small frame,
 * a 32 x 16 panorama at k = 2 is 8 blocks on a device of 256 CUs, and an irradiance volume is a thousand of them.  The frames share everything
 * of `view` but the camera: model, width, height, k, half_w, half_h, half_angle, t_min, t_max, tone, flags.
 * DEFINITION, by composition.  R = width * height * k * k, P = width * height.  The buffers are n_frames frames back to back: frame f owns rays
 * and seeds [f * R, (f + 1) * R) and radiance and pixel [f * P, (f + 1) * P).  Frame f ends, bit for bit in every buffer the caller passes, as
 * after the single call -- mirt_view_rays for the rays, mirt_render_view for seeds, radiance and pixel, MIRT_VIEW_ACCUMULATE, tone and the dead
 * FISHEYE samples included -- on buffers holding just that slice, with a descriptor equal to *view but eye / right / up / forward = cameras[f].
 * Both libraries give the same bits, as for the single call.  view->eye / right / up / forward are neither read nor checked.
 * `cameras` is a HOST array of n_frames entries, borrowed for the call like every host pointer of this header, and so checked completely before
 * anything is queued; the call copies it to device memory of the context in stream order, so a batch call queued behind a running one does not
 * disturb the table that one reads.  (A caller with cameras in device memory brings them to the host: 48 bytes a frame.)
 * mirt_view_deferred reports mirt_render_view_batch as it reports mirt_render_view: the rays re-run in the exact kernel, in whole blocks of 256
 * (a block may hold rays of two frames).
 * CHECKS, all before anything is queued; nothing is written when one fails, and the context works afterwards.  MIRT_E_ARG: everything
 * mirt_view_rays / mirt_render_view refuse in the descriptor except the basis; row0 != 0, or nrows neither 0 nor height (whole frames only);
 * cameras NULL with n_frames > 0; a non-finite component in any camera (the message names the frame); n_frames * R above 2^32 - 256; the overlap
 * rules of mirt_render_view on the whole batch buffers; a call while capturing.  MIRT_E_RANGE: a buffer shorter than n_frames frames, a material
 * table shorter than one entry.  MIRT_E_DATA and MIRT_E_HANDLE as in the single call.  n_frames == 0 is MIRT_OK and queues nothing.  A held
 * command stream is flushed first; wrapped geometry is re-validated once per call.
 * KERNELS: k_viewRaysBatch and k_viewPassBatch (csrc/pt_kernels_view_batch.hip: the text of k_viewRays and k_viewPass, csrc/pt_view_kernels.inc,
 * with the compile-time flag BATCH set, in a translation unit of their own) -- the stacked frames are one image of n_frames * height
 * rows to them; a lane takes its frame from its row and loads that camera from the table (csrc/pt_view.hpp).  The single calls keep their code.
 * The batch's guides and ambient occlusion: mirt_view_guides_batch, mirt_render_view_guided_batch, mirt_view_ao_batch, below.
 * NOT BUILT: row tiles of a batch; frames that differ in model, size or k; cameras in device memory; graph capture.
 * MIRT_ABI_VERSION is unchanged: a host detects the entry points by their symbols. */
typedef struct mirt_view_camera { float eye[3], right[3], up[3], forward[3]; } mirt_view_camera;   /* 48 bytes */
MIRT_API int mirt_view_rays_batch(mirt_ctx* ctx, const mirt_view_desc* view, const mirt_view_camera* cameras, uint32_t n_frames, mirt_buf* rays);
MIRT_API int mirt_render_view_batch(mirt_ctx* ctx, const mirt_pass_desc* scene, const mirt_view_desc* view, const mirt_view_camera* cameras,
                                    uint32_t n_frames, mirt_buf* seeds, mirt_buf* radiance, mirt_buf* pixel);
/* FIRST-HIT GUIDES OF A VIEW CAMERA'S TILE, one launch: what mirt_render_guides is to the thin lens, for the cameras above -- the two float4
 * images per pixel that mirt_filter_atrous and mirt_upsample_guided consume, whichever camera made them.
 * DEFINITION, by composition.  Pixel p of the tile has the rays p * rpp + i, i = 0 .. rpp - 1, exactly as mirt_view_rays writes them.  Each runs
 * with a Poi reset as initTrace resets it through sphereTrace, triangleTrace and every meshTrace in upload order: mirt_trace_closest's CLOSEST.
 * A sample is a HIT iff 0 <= Poi.matId < the number of material entries (mirt_render_guides's rule: an id past the table is not a hit and reads
 * nothing -- so the material buffer is needed even when only normal_hits is asked for).
 *   normal_hits [p] = float4(sum Poi.normal.x, sum .y, sum .z, number of hit samples)
 *   albedo_depth[p] = float4(sum material[matId].x, sum .y, sum .z, sum Ray.maxt)
 * sequential fp32 sums from +0 over the hit samples in sample order; a pixel without a hit is all +0 in both.  A DEAD fisheye sample (r > 1)
 * enters dead and is never a hit: a pixel wholly outside the circle is background for the filter.  DEPTH IS IN UNITS OF |d|, as the ray
 * queries report t: `forward` and the basis are used as given, so an ORTHOGRAPHIC camera with |forward| = 2 reports half the distance.  k = 1 is
 * allowed here, unlike rays_per_pixel == 1 in mirt_render_guides: these cameras draw nothing from the seeds.
 * Of `scene` only struct_size, the primitive sets and material are read; of `view` everything but tone and the meaning of flags (an unknown
 * flag is still refused).  Nothing but the two outputs is written.  Positions use the global y: a tile's guides equal the same rows of the frame's.
 * CHECKS, all before anything is queued; nothing is written when one fails.  MIRT_E_ARG: mirt_view_rays's descriptor checks, a wrong struct_size
 * of `scene`, both outputs NULL, an output whose bytes meet the other's, a geometry buffer's or the material's, the mesh count rule of
 * mirt_trace_radiance, a call while capturing.  MIRT_E_RANGE: an output shorter than the tile's pixels x 16 B, a material table shorter than one
 * entry.  MIRT_E_DATA: a cell table that fails validation.  MIRT_E_HANDLE: a bad context or buffer.  A held command stream is flushed first;
 * wrapped geometry is re-validated as for a pass.
 * KERNEL (csrc/pt_kernels_rays.hip k_viewGuides): one lane per pixel walking its samples in order -- by default the optimistic / exact pair PER
 * PIXEL, a bit per pixel; mirt_ctx_set_exact_only is honoured.  MIRT_ABI_VERSION is unchanged: a host detects the entry point by its symbol. */
MIRT_API int mirt_view_guides(mirt_ctx* ctx, const mirt_pass_desc* scene, const mirt_view_desc* view, mirt_buf* normal_hits, mirt_buf* albedo_depth);
/* THE FRAME AND ITS GUIDES in one call.  Every buffer the caller passes -- seeds, radiance, pixel, normal_hits, albedo_depth -- ends bit for bit
 * as after mirt_render_view(ctx, scene, view, seeds, radiance, pixel) followed by mirt_view_guides(ctx, scene, view, normal_hits, albedo_depth),
 * with or without MIRT_VIEW_ACCUMULATE: the guides are the same for every progressive pass, so a host takes them with the first and renders the
 * later ones plain.  CHECKS: those of both calls, plus a guide buffer whose bytes meet the seeds', the radiance's or the pixel's (MIRT_E_ARG),
 * all before anything is queued -- when one fails nothing is written at all.  mirt_view_deferred means what it means after mirt_render_view.
 * ROUTE.  ONE LAUNCH (per kernel of the optimistic / exact pair) where a pixel's samples are consecutive lanes of one wave -- rpp 1, 4, 16 or
 * 64, k = 1, 2, 4 or 8: the frame's kernel adds a pixel's eight values lane by lane right after its camera rays' closest-hit stage and writes
 * the guides itself.  EVERYWHERE ELSE -- k = 16, where a pixel spans four waves, and MIRT_GUIDED_VIEW=0 in the environment (an A/B switch, read
 * per call) -- the call queues the two calls' launches.  mirt_ctx_guided_views: the calls of this context that took the one-launch route.
 * The optimistic kernel writes a block's guides before its verdict; a block that defers is re-run whole by the exact kernel, which writes the
 * same pixels' guides again, later on the same stream.  The outputs are therefore FINAL IN STREAM ORDER -- when the call's launches have
 * completed (mirt_finish) -- like every other output of the frame, not before.  Not built: a one-launch route at k = 16, graph capture.
 * MIRT_ABI_VERSION is unchanged: a host detects the entry points by their symbols. */
MIRT_API int mirt_render_view_guided(mirt_ctx* ctx, const mirt_pass_desc* scene, const mirt_view_desc* view, mirt_buf* seeds, mirt_buf* radiance,
                                     mirt_buf* pixel, mirt_buf* normal_hits, mirt_buf* albedo_depth);
MIRT_API int mirt_ctx_guided_views(mirt_ctx* ctx, uint64_t* count);
/* AMBIENT OCCLUSION OF THE FIRST HIT of the row tile, in one launch: the AOV the guides lack.  ao_out holds one uint32[2] per tile-local pixel,
 * {open, cast}, 8 bytes per pixel.  Pixel p of the row tile has the rays p * rays_per_pixel + i, i = 0 .. rays_per_pixel - 1, each taken as
 * initTrace and the closest-hit stage leave it -- sphereTrace, triangleTrace, then every meshTrace in upload order -- before lightRender: exactly
 * the guides' state (mirt_render_guides).
 *   A sample CASTS iff Poi.matId >= 0: bouncePaths' own test (A10 code.cl:592).  No material is read, an id past the table casts too.
 *   A casting sample starts with s = seeds[local ray] and makes `samples` AO rays, j = 0 .. samples - 1: AO ray j is the ray
 *   getHemisphereRay(poi, &s) returns (code.cl:545-579) -- what the j-th of `samples` consecutive bouncePaths calls on the unchanged Poi buffer,
 *   with the seeds advancing, would store -- then given maxt = radius and, when bias != 0, the origin o.c = p.c + (n.c * bias) per component:
 *   two fp32 operations, each rounded on its own, not an fma.  bias == 0: the origin is Poi.p bit for bit.
 *   The AO ray is OCCLUDED by mirt_trace_occluded's definition: mint == maxt after sphereShadowTrace, triangleShadowTrace and a
 *   triangleShadowTrace per mesh in upload order.
 *   cast = the number of AO rays made for the pixel (casting samples x `samples`); open = the number of those that are not occluded.  Both are
 *   integers, so no summation order is involved; a pixel with no hit is {0, 0}.  The lights play no part: an emitter in front of the surface
 *   is not considered, as in the guides.
 * READ AND WRITTEN.  `seeds` is read and NEVER written: AO does not advance the frame's random sequence.  Tile-local buffers with global ray ids,
 * as in a pass: a tile's AO equals the same rows of the whole frame's.  Nothing but ao_out is written.  Reads of the descriptor: the image size,
 * rays_per_pixel, row0 / nrows, cam, scene_bounds, focal_length, lens_rad, the primitive sets and seeds.  Ignored, and free to be NULL or 0: acu,
 * pixel, radiance, material, the lights, bounces, pass_index.
 * CHECKS, all before anything is queued; nothing is written when one fails, and the context works afterwards.  MIRT_E_ARG: a wrong struct_size in
 * either descriptor, samples 0 or above MIRT_AO_MAX_SAMPLES, radius NaN or <= 0 (+inf is allowed), bias negative, NaN or infinite,
 * rays_per_pixel that is not k x k, or 1 (the guides' rule: its lens sample draws from seeds[col]), a tile outside the image or of more than
 * 2^32 - 256 rays, NULL seeds or ao_out, ao_out whose bytes meet the seeds' or a geometry buffer's, a call while capturing.  MIRT_E_RANGE: seeds
 * shorter than the tile's rays x 4 B, ao_out shorter than the tile's pixels x 8 B.  MIRT_E_DATA: a cell table that fails validation.
 * MIRT_E_HANDLE: a bad context or buffer.  A held command stream (mirt_ctx_set_fusion, frame fusion) is flushed first; wrapped geometry is
 * re-validated as for a pass.
 * KERNEL.  One launch, one lane per pixel walking its samples in order (csrc/pt_kernels_rays.hip k_ao) -- by default the optimistic / exact
 * pair PER PIXEL, as for the guides: a pixel one of whose primary or AO rays the ray-side guard refuses, or whose grid walk defers, is redone
 * whole by the exact kernel; mirt_ctx_set_exact_only is honoured.  mirt_ao_deferred: the pixels the last mirt_render_ao re-ran in the exact
 * kernel, counted when asked, like mirt_trace_deferred.  MIRT_ABI_VERSION is unchanged: a host detects the entry points by their symbols. */
#define MIRT_AO_MAX_SAMPLES 64u
#define MIRT_AO_DEFAULT_SAMPLES 4u
#define MIRT_AO_DEFAULT_BIAS 0.001f      /* initShadowTrace's own displacement, A10 code.cl:659 */
typedef struct mirt_ao_desc {
    uint32_t struct_size;           /* sizeof(mirt_ao_desc)                                        */
    uint32_t samples;               /* AO rays per hit primary sample, 1 .. MIRT_AO_MAX_SAMPLES     */
    float radius;                   /* the AO ray's maxt; > 0, +inf allowed                        */
    float bias;                     /* >= 0, finite; 0: the origin is Poi.p bit for bit            */
} mirt_ao_desc;
MIRT_API int mirt_render_ao(mirt_ctx* ctx, const mirt_pass_desc* desc, const mirt_ao_desc* ao, mirt_buf* ao_out);
MIRT_API int mirt_ao_deferred(mirt_ctx* ctx, uint64_t* pixels);
/* AMBIENT OCCLUSION OF A VIEW CAMERA'S TILE, one launch: what mirt_render_ao is to the thin lens, for the panoramic, fisheye and orthographic
 * cameras.  ao_out holds one uint32[2] per tile-local pixel, {open, cast}, 8 bytes per pixel.
 * DEFINITION, by composition.  Pixel p of the tile has the rays p * rpp + i, i = 0 .. rpp - 1, rpp = k * k, exactly as mirt_view_rays writes
 * them (global y; a DEAD fisheye sample enters dead).  Each runs as mirt_trace_closest's CLOSEST: a Poi reset as initTrace resets it, then
 * sphereTrace, triangleTrace and every meshTrace in upload order.  From there on the words are mirt_render_ao's, above: a sample CASTS iff
 * Poi.matId >= 0 (no material is read, an id past the table casts too; a dead or missing sample casts nothing); a casting sample starts with
 * s = seeds[tile-local ray id] and makes ao->samples AO rays, ray j what getHemisphereRay(poi, &s) returns, then given maxt = radius and, when
 * bias != 0, the origin o.c = p.c + (n.c * bias) -- two fp32 operations, each rounded on its own; bias == 0: Poi.p bit for bit; the AO ray is
 * OCCLUDED by mirt_trace_occluded's definition; cast = casting samples x samples, open = the number of those rays not occluded; a pixel with no
 * hit is {0, 0}.
 * READ AND WRITTEN.  `seeds` (int32 per tile ray) is read and NEVER written.  Of `scene` only struct_size and the primitive sets are read: no
 * material, no lights.  Of `view` everything but tone and the meaning of flags (an unknown flag is still refused).  k = 1 is allowed: these
 * cameras draw nothing from the seeds.  Nothing but ao_out is written.  A tile's AO equals the same rows of the frame's when its seeds carry the
 * global ids (mirt_seed_fill with first = row0 * width * rpp).
 * CHECKS, all before anything is queued; nothing is written when one fails, and the context works afterwards.  MIRT_E_ARG: mirt_view_rays's
 * descriptor checks, a wrong struct_size in any of the three descriptors, samples 0 or above MIRT_AO_MAX_SAMPLES, radius NaN or <= 0 (+inf is
 * allowed), bias negative, NaN or infinite, NULL seeds or ao_out, ao_out whose bytes meet the seeds' or a geometry buffer's, the mesh count rule
 * of mirt_trace_radiance, a call while capturing.  MIRT_E_RANGE: seeds shorter than the tile's rays x 4 B, ao_out shorter than the tile's
 * pixels x 8 B.  MIRT_E_DATA: a cell table that fails validation.  MIRT_E_HANDLE: a bad context or buffer.  A held command stream is flushed
 * first; wrapped geometry is re-validated as for a pass.
 * KERNEL (csrc/pt_kernels_rays.hip k_viewAo; the argument rules csrc/pt_view_plan.hpp view_check_ao): one lane per pixel walking its samples in
 * order -- by default the optimistic / exact pair PER PIXEL, a bit per pixel; mirt_ctx_set_exact_only is honoured.  mirt_view_ao_deferred: the
 * pixels the last mirt_view_ao re-ran in the exact kernel, counted when asked, like mirt_ao_deferred.  Not built: AO folded into the frame's own
 * launch, graph capture.  MIRT_ABI_VERSION is unchanged: a host detects the entry points by their symbols. */
MIRT_API int mirt_view_ao(mirt_ctx* ctx, const mirt_pass_desc* scene, const mirt_view_desc* view, const mirt_ao_desc* ao, mirt_buf* seeds, mirt_buf* ao_out);
MIRT_API int mirt_view_ao_deferred(mirt_ctx* ctx, uint64_t* pixels);
/* GUIDES AND AMBIENT OCCLUSION OF THE BATCHED VIEW CAMERAS: what an irradiance volume needs beside radiance per probe -- the distance to the
 * first hit (the visibility term), normals and albedo, ambient occlusion -- for n_frames cameras in ONE call and one launch (pair).
 * DEFINITION, by composition, exactly as for mirt_render_view_batch.  R = width * height * k * k, P = width * height.  The buffers are n_frames
 * frames back to back: frame f owns seeds [f * R, (f + 1) * R) and radiance, pixel, normal_hits, albedo_depth and ao_out [f * P, (f + 1) * P).
 * Frame f ends, bit for bit in every buffer the caller passes, as after the single call -- mirt_view_guides, mirt_render_view_guided,
 * mirt_view_ao -- on buffers holding just that slice, with a descriptor equal to *view but eye / right / up / forward = cameras[f].  Both
 * libraries give this against their own single calls.  view->eye / right / up / forward are neither read nor checked.  AO seeds are read and
 * never written.  In the guided call MIRT_VIEW_ACCUMULATE, tone and the dead FISHEYE samples behave as in the single call.
 * CHECKS, all before anything is queued; nothing is written when one fails, and the context works afterwards.  First the batch's, in
 * mirt_render_view_batch's order: whole frames only, n_frames * R <= 2^32 - 256, cameras NULL with n_frames > 0, a non-finite camera component
 * (the message names the frame).  Then the single call's own, in its order: both guides NULL; the AO descriptor's rules, NULL seeds, NULL
 * ao_out; for the guided call the frame's rules and then both guides NULL.  The overlap rules are the single calls', on the whole batch
 * buffers.  MIRT_E_RANGE: a buffer shorter than n_frames frames.  MIRT_E_DATA, MIRT_E_HANDLE and a call while capturing as in the single calls.
 * n_frames == 0 is MIRT_OK and queues nothing.
 * COUNTERS.  mirt_view_ao_deferred reports the last mirt_view_ao_batch as it reports mirt_view_ao (pixels); mirt_view_deferred the guided batch
 * as the plain batch; mirt_ctx_guided_views counts a guided batch call that took the one-launch route once.
 * KERNELS (csrc/pt_kernels_view_batch.hip): k_viewGuidesBatch and k_viewAoBatch, the text of k_viewGuides and k_viewAo
 * (csrc/pt_view_aov_kernels.inc) with the camera from the table -- one lane and one mask bit per pixel of the image of n_frames * height rows,
 * the optimistic / exact pair PER PIXEL.  The guided call's ROUTE is mirt_render_view_guided's: k_viewPassBatch writes the guides itself at
 * k = 1, 2, 4 or 8; at k = 16 and under MIRT_GUIDED_VIEW=0 the call queues the plain batch's launches and then the guide batch's.  The outputs
 * are final in stream order, as documented there.
 * NOT BUILT: row tiles of a batch; frames that differ in model, size or k; cameras in device memory; a one-launch guided route at k = 16; AO
 * folded into the frame's launch; filtering a batch (the a-trous filter would have to stop at frame borders); graph capture.
 * MIRT_ABI_VERSION is unchanged: a host detects the entry points by their symbols. */
MIRT_API int mirt_view_guides_batch(mirt_ctx* ctx, const mirt_pass_desc* scene, const mirt_view_desc* view, const mirt_view_camera* cameras,
                                    uint32_t n_frames, mirt_buf* normal_hits, mirt_buf* albedo_depth);
MIRT_API int mirt_render_view_guided_batch(mirt_ctx* ctx, const mirt_pass_desc* scene, const mirt_view_desc* view, const mirt_view_camera* cameras,
                                           uint32_t n_frames, mirt_buf* seeds, mirt_buf* radiance, mirt_buf* pixel, mirt_buf* normal_hits,
                                           mirt_buf* albedo_depth);
MIRT_API int mirt_view_ao_batch(mirt_ctx* ctx, const mirt_pass_desc* scene, const mirt_view_desc* view, const mirt_view_camera* cameras,
                                uint32_t n_frames, const mirt_ao_desc* ao, mirt_buf* seeds, mirt_buf* ao_out);
/* Edge-avoiding A-TROUS FILTER of a few-rays-per-pixel frame, guided by the first-hit guide buffers: `radiance` as a pass writes it (un-scaled
 * sums), `normal_hits` and `albedo_depth` as mirt_render_guides writes them, all float4 per pixel of a width x height image -- a whole frame, or a
 * gathered one.  Everything stays on the device; the working images live in the context's scratch buffer.
 *
 * DEFINITION.  Every operation below is ONE fp32 operation rounded on its own, in the order written; nothing is a fused multiply-add; every `/`
 * is the correctly rounded fp32 quotient; max(a, b) is v_max_f32 (a NaN loses).  R = radiance, (N, hits) = normal_hits, (A, D) = albedo_depth.
 *   Per pixel p:   p is LIVE iff hits > 0.  For a live p: r = 1 / hits, n^ = N * r, z = D * r, a = A * r.
 *                  I_0 = R.xyz.  With MIRT_FILTER_DEMODULATE, for a live p and per channel c: I_0.c = R.c / a.c where a.c > 0; elsewhere the
 *                  channel is left alone and a.c counts as 1 on the way back.
 *   A pixel that is not live (background) keeps I_0 through every iteration and is never a tap.
 *   Iteration i = 0 .. iterations - 1, step s = 2^i, live p:
 *     the centre first:  sumw = 0.140625, sumc = I_i(p) * 0.140625   (the B3 spline h = (1/16, 1/4, 3/8, 1/4, 1/16): exactly h[0]^2; no edge
 *                        term is evaluated for the centre)
 *     the other 24 taps q = p + s * (dx, dy), dy = -2 .. 2 outer, dx = -2 .. 2 inner; a tap outside [0, width) x [0, height) or not live is
 *     skipped; otherwise
 *       k  = h[|dy|] * h[|dx|]
 *       dn = max(0, (n^p.x * n^q.x + n^p.y * n^q.y) + n^p.z * n^q.z);  wn = dn squared normal_power_log2 times
 *       wz = max(0, 1 - |zp - zq| * izp),  izp = 1 / (sigma_depth * zp) once per centre pixel;          wz = 1 when the term is off
 *       e  = (I_i(p) - I_i(q)) * tone per channel,  c = (e.x * e.x + e.y * e.y) + e.z * e.z,
 *       wc = max(0, 1 - c * inv_i),  inv_i = 1 / (k_i * k_i), k_i = sigma_colour * 2^-i (on the host, IEEE fp32);   wc = 1 when the term is off
 *       w  = ((k * wn) * wz) * wc
 *       only when w > 0 (false for a NaN):  sumw += w,  sumc += I_i(q) * w per channel
 *     I_{i+1}(p) = sumc / sumw per channel.
 *   End: out = I_n, per channel times a.c where the pixel was demodulated by it.  filtered = (out.xyz, R.w).  pixel = copyToPixel's own tone map
 *   (A10 code.cl:1381-1385): clamp((out * (255 * tone)) * 1.8, 0, 255) converted like the pass's (truncate, NaN -> 0), alpha 255.
 * A term is OFF when its sigma is <= 0, NaN or infinite.  `tone` is the float m copyToPixel takes, 1 / (rays_per_pixel * passes).
 * What follows: with iterations == 0 and no DEMODULATE, filtered == radiance bit for bit and pixel == the pixel buffer the pass itself wrote;
 * with the colour term on, a NaN or infinite pixel stays where it is and does not spread (its c is not a number below 1, so it is nobody's tap and has none);
 * background pixels come out as they went in.  libmirt.so and libmirt_default.so give the same bits: the reference has no filter, there is one
 * contract (csrc/pt_kernels_filter.hip says how the quotients are formed).
 * This call has NO TILES: rows near a tile border need the neighbour's rows, so filtering row tiles separately gives a different picture within
 * 2 * (2^iterations - 1) rows of a border.  With N devices, either gather radiance and both guides to one context and filter there, or exchange
 * the halo rows and filter every tile where it is (mirt_exchange_rows, mirt_filter_atrous_rows, below): the same bits.
 * Checks, nothing is written when one fails.  MIRT_E_ARG: struct_size, width or height 0 or above 65535, iterations > MIRT_FILTER_MAX_ITERATIONS,
 * normal_power_log2 > MIRT_FILTER_MAX_NORMAL_POWER_LOG2, tone not finite or <= 0, unknown flags or both structure flags, both outputs NULL, an
 * output that is (or overlaps) an input or the other output, a call while capturing.  MIRT_E_RANGE: a buffer smaller than width * height elements.
 * MIRT_E_HANDLE: a bad context or buffer.  The call observes device state: a held command stream (mirt_ctx_set_fusion, frame fusion) is flushed first.
 * MIRT_ABI_VERSION is unchanged: a host detects the entry point by its symbol. */
#define MIRT_FILTER_DEMODULATE 1u       /* filter radiance / albedo and multiply the albedo back: texture and colour borders stay sharp   */
/* An iteration runs as one of two kernels with identical results -- one thread per pixel reading its taps through the caches, or LDS tiles of
 * the step's sub-lattice -- chosen per step size from measurements.  These force one for every step: for measurement. */
#define MIRT_FILTER_DIRECT 2u
#define MIRT_FILTER_TILED 4u
#define MIRT_FILTER_MAX_ITERATIONS 5u
#define MIRT_FILTER_MAX_NORMAL_POWER_LOG2 7u
/* the parameters the hosts ship as defaults (Python Context.filter_atrous, Node queue.filterFrame, cli.js --denoise), with MIRT_FILTER_DEMODULATE */
#define MIRT_FILTER_DEFAULT_ITERATIONS 3u
#define MIRT_FILTER_DEFAULT_NORMAL_POWER_LOG2 5u
#define MIRT_FILTER_DEFAULT_SIGMA_DEPTH 0.1f
#define MIRT_FILTER_DEFAULT_SIGMA_COLOUR 1.0f
typedef struct mirt_filter_desc {
    uint32_t struct_size;           /* sizeof(mirt_filter_desc)                                    */
    uint32_t width, height;         /* of the buffers the caller holds                             */
    uint32_t iterations;            /* 0 .. 5; iteration i uses step 2^i                           */
    uint32_t flags;                 /* MIRT_FILTER_*                                               */
    uint32_t normal_power_log2;     /* 0 .. 7                                                      */
    float tone;                     /* 1 / (rays_per_pixel * passes)                               */
    float sigma_depth, sigma_colour;/* <= 0, NaN or inf: that term is off                          */
    mirt_buf* radiance;             /* in:  float4 per pixel                                       */
    mirt_buf* normal_hits;          /* in:  float4 per pixel                                       */
    mirt_buf* albedo_depth;         /* in:  float4 per pixel                                       */
    mirt_buf* filtered;             /* out: float4 per pixel, un-scaled like radiance; may be NULL */
    mirt_buf* pixel;                /* out: uchar4 per pixel; may be NULL (not both)               */
} mirt_filter_desc;
MIRT_API int mirt_filter_atrous(mirt_ctx* ctx, const mirt_filter_desc* desc);
/* GUIDE-DRIVEN UPSAMPLING: shade at 1/f resolution, output at full.  The radiance of a wl x hl frame, wl = width / factor, hl = height / factor
 * (`radiance_lo`: what a pass wrote as `radiance` or mirt_filter_atrous as `filtered`, un-scaled sums), is rebuilt at width x height by a
 * joint-bilateral interpolation of its four nearest low pixels, weighted by the first-hit guides of BOTH resolutions (mirt_render_guides at
 * wl x hl and at width x height) and re-modulated with the full-resolution albedo, so that geometric and material borders land on full-resolution
 * pixels.  The camera's window is given in scene space (A10 code.cl:93-98), so the same camera at wl x hl covers the same frustum and low pixel
 * (X, Y) covers the factor x factor high pixels under it: the sizes must be exact multiples of factor.  The two guide pairs may come from
 * different ray counts: each is normalised by its own hit count.  `tone` is the low frame's 1 / (rays_per_pixel * passes).
 *
 * DEFINITION, in the conventions of mirt_filter_atrous: every operation below is ONE fp32 operation rounded on its own, in the order written;
 * nothing is a fused multiply-add; every `/` is the correctly rounded fp32 quotient; max(a, b) is v_max_f32 (a NaN loses).  f = factor.
 *   Per low pixel q:   R_lo = radiance_lo, (N_lo, hits_lo) = normal_hits_lo, (A_lo, D_lo) = albedo_depth_lo.  q is LIVE iff hits_lo > 0; then
 *                      r = 1 / hits_lo, n^q = N_lo * r, zq = D_lo * r, aq = A_lo * r.  Tap value per channel c: J(q).c = R_lo.c / aq.c where q is
 *                      live, MIRT_UPSAMPLE_DEMODULATE is set and aq.c > 0; otherwise J(q).c = R_lo.c.
 *   Per high pixel p = (x, y):   p is LIVE iff hits > 0; then n^p, zp, ap likewise from normal_hits / albedo_depth, and
 *                      izp = 1 / (sigma_depth * zp).  The depth term is OFF when sigma_depth is <= 0, NaN or infinite.
 *   Tap geometry, in integers, per axis (csrc/pt_upsample_taps.hpp):  e = 2x + 1 - f;  X0 = floor(e / 2f) (floor: -1 at the left edge);
 *                      m = e - 2f * X0 in [0, 2f);  tx = (float)m / (float)(2f);  bx[0] = 1 - tx, bx[1] = tx.  The same for y.
 *   Live p: the taps q = (X0 + i, Y0 + j), j = 0, 1 outer, i = 0, 1 inner; a tap outside the low image or not live is skipped; otherwise
 *       b  = by[j] * bx[i]
 *       dn = max(0, (n^p.x * n^q.x + n^p.y * n^q.y) + n^p.z * n^q.z);  wn = dn squared normal_power_log2 times
 *       wz = max(0, 1 - |zp - zq| * izp);          wz = 1 when the term is off
 *       w  = (b * wn) * wz
 *       only when w > 0 (false for a NaN):  sumw += w,  sumc += J(q) * w per channel; both sums start at +0.
 *   Background p (not live): the same four taps, but only taps that are NOT live count; w = b (counted only when w > 0), tap value R_lo.xyz.
 *   When sumw > 0:  I = sumc / sumw per channel.
 *   FALLBACK, for either kind of p, when sumw > 0 is false (a surface the low frame does not have, weights that are all 0 or NaN):
 *       Q0 = (x div f, y div f);  I = J(Q0) when p and Q0 are both live; otherwise I = R_lo(Q0).xyz and nothing is multiplied back.
 *   End: for a live p that did not take the raw fallback, per channel: out.c = I.c * ap.c where the flag is set and ap.c > 0; otherwise
 *   out.c = I.c.  upsampled = (out.xyz, R_lo(Q0).w).  pixel = copyToPixel's own tone map of out, exactly as mirt_filter_atrous's.
 * What follows, and what does not.  Inside the low image the b of the four taps are those of plain bilinear interpolation between low pixel
 * centres, clamped at the border (an outside tap is dropped and the division by sumw renormalises).  There is NO colour term here, so a NaN or
 * infinite low pixel is NOT contained the way the filter contains one: it reaches every high pixel that counts it as a tap (up to (2f)^2 of them),
 * with the depth term on or off; only `w > 0` keeps a NaN WEIGHT out.  libmirt.so and libmirt_default.so give the same bits: the reference has
 * no upsampler, there is one contract (csrc/pt_kernels_upsample.hip).
 * This call wants whole frames; row tiles are mirt_upsample_guided_rows (below).  NOT built: a footprint wider than 2 x 2 taps, a colour term, an
 * LDS-tiled structure, sizes that factor does not divide.
 * Checks, nothing is written when one fails.  MIRT_E_ARG: struct_size, width or height 0 or above 65535, factor outside 2 .. 4, a size that is not
 * a multiple of factor, normal_power_log2 > MIRT_FILTER_MAX_NORMAL_POWER_LOG2, tone not finite or <= 0, unknown flags, both outputs NULL, an
 * output that is (or overlaps) an input or the other output, a call while capturing.  MIRT_E_RANGE: a buffer smaller than its image.
 * MIRT_E_HANDLE: a bad context or buffer.  A held command stream (mirt_ctx_set_fusion, frame fusion) is flushed first.
 * MIRT_ABI_VERSION is unchanged: a host detects the entry point by its symbol. */
#define MIRT_UPSAMPLE_DEMODULATE 1u     /* interpolate radiance / albedo of the low frame and multiply the full-resolution albedo back */
#define MIRT_UPSAMPLE_MIN_FACTOR 2u
#define MIRT_UPSAMPLE_MAX_FACTOR 4u
/* the parameters the hosts ship as defaults (Python Context.upsample_guided, Node queue.upsampleFrame, cli.js --upscale), with MIRT_UPSAMPLE_DEMODULATE */
#define MIRT_UPSAMPLE_DEFAULT_NORMAL_POWER_LOG2 5u
#define MIRT_UPSAMPLE_DEFAULT_SIGMA_DEPTH 0.1f
typedef struct mirt_upsample_desc {
    uint32_t struct_size;           /* sizeof(mirt_upsample_desc)                                          */
    uint32_t width, height;         /* the HIGH resolution: of normal_hits, albedo_depth and the outputs   */
    uint32_t factor;                /* 2 .. 4; the low images are (width / factor) x (height / factor)     */
    uint32_t flags;                 /* MIRT_UPSAMPLE_*                                                     */
    uint32_t normal_power_log2;     /* 0 .. 7                                                              */
    float tone;                     /* the low frame's 1 / (rays_per_pixel * passes)                       */
    float sigma_depth;              /* <= 0, NaN or inf: the depth term is off                             */
    mirt_buf* radiance_lo;          /* in:  float4 per low pixel                                           */
    mirt_buf* normal_hits_lo;       /* in:  float4 per low pixel                                           */
    mirt_buf* albedo_depth_lo;      /* in:  float4 per low pixel                                           */
    mirt_buf* normal_hits;          /* in:  float4 per high pixel                                          */
    mirt_buf* albedo_depth;         /* in:  float4 per high pixel                                          */
    mirt_buf* upsampled;            /* out: float4 per high pixel, un-scaled like radiance; may be NULL    */
    mirt_buf* pixel;                /* out: uchar4 per high pixel; may be NULL (not both)                  */
} mirt_upsample_desc;
MIRT_API int mirt_upsample_guided(mirt_ctx* ctx, const mirt_upsample_desc* desc);
/* Two ways to run the pass, identical results.  Default: the optimistic pair -- a kernel whose divisions are 3-operation
 * forms proven bit-exact inside a guard window (exhaustively, on the device: profiles/r1_divcheck_exhaustive.txt), plus the
 * exact kernel re-running the samples whose rays left the window (NaN rays, axis-parallel directions, ...); it needs every
 * grid to pass the geometry-side window check, otherwise the pass silently is the exact one.  mirt_ctx_set_exact_only(ctx, 1):
 * one kernel whose every division is the compiler's correctly rounded expansion.  The pair is queued without a host round trip
 * (the exact kernel walks the optimistic kernel's bit mask on the device).  mirt_pass_deferred: how many samples the last pass
 * re-ran through the exact kernel -- counted when asked (one small launch + a stream sync), valid until the next pass. */
MIRT_API int mirt_pass_deferred(mirt_ctx* ctx, uint64_t* samples);
MIRT_API int mirt_ctx_set_exact_only(mirt_ctx* ctx, int on);

/* Command-stream fusion: the reference host's pass, kernel by kernel, at the fused pass's speed -- with no change to the host.
 * executeRender (A10 code.js:1806-1854) issues a pass as 44+ enqueues whose every stage round-trips Ray / Poi / shadow Ray / acu
 * through HBM (4.2 KB per sample; the fused pass moves 24 B).  At level 2 the runtime holds back the enqueues of the Assign10 pass
 * kernels from an initTrace on, and when the stream up to the copyToPixel IS executeRender's sequence over one consistent set of
 * buffers and arguments -- initTrace; sphere / triangle / mesh Trace; lightRender per light; per light {initShadowTrace, the
 * any-hit kernel of every set, sceneRender}; any number of {bouncePaths, closest-hit kernels, that per-light block}; copyToPixel --
 * it runs as ONE launch of the fused pass + the recorded copyToPixel.  Anything else is launched enqueue by enqueue, in order,
 * exactly as at level 0: a different kernel order, mixed buffers or changed geometry arguments inside the pass, a global size
 * smaller than the ray count, and any command that observes or changes device state while enqueues are held (buffer read / write /
 * release, mirt_zero, mirt_seed_fill, mirt_render_pass, capture, timers, gather, destroy ...) flush the held stream first.
 * What level 2 trades, and why it is off by default in this ABI (the WebCL object model above it turns it on: end of this comment):
 *   - seeds, acu and pixel after the pass are bit-identical to level 0 (tests/test_fusion.py replays the reference host's own call
 *     stream both ways); the Ray, Poi and shadow-Ray buffers are NOT written by a fused pass -- they keep their previous contents.
 *     The reference host never reads them (it cannot: it does not know their layout beyond sizeof).
 *   - mirt_finish inside a held pass returns without draining anything (the reference calls finish() after every sceneRender,
 *     code.js:1406); the work runs at the copyToPixel.  Host-side timing of individual kernels is therefore meaningless.  A held pass
 *     that involves a wrapped buffer (mirt_buf_wrap: memory the caller can reach behind the ABI) IS drained by mirt_finish, and
 *     mirt_buf_device_ptr drains whatever is held.
 *   - errors of a held enqueue (a buffer too small, a grid failing validation) are reported by the call that flushes it, and the
 *     held enqueues after the failing one are dropped (at level 0 the host would have stopped at that enqueue's exception).
 * Level 0 (the default of mirt_ctx_create): every enqueue launches its kernel.  The environment variable MIRT_FUSION=0|2 sets the level
 * of every new context.  The WebCL object model above this ABI (host/webcl.js webcl.createContext) asks for level 2 itself unless the
 * variable is set: its one client, the reference page, cannot observe the difference.
 * mirt_ctx_fused_passes: how many passes of this context ran fused. */
MIRT_API int mirt_ctx_set_fusion(mirt_ctx* ctx, int level);
MIRT_API int mirt_ctx_fused_passes(mirt_ctx* ctx, uint64_t* count);

/* ---- extension: a whole Assign04 / Assign07 frame in one launch ------------------------------------
 * One call == compute() / computeTri() / computeBoth() of those pages minus the read-back (A04 code.js:553-577, A07 code.js:571-661): initTrace and
 * the trace kernel(s) on one thread per pixel, the primary ray in registers.  Kernel by kernel a frame is two or three launches with a 48-byte ray per
 * pixel written and read back between them; here nothing per ray touches memory unless `rays` is given.  `pixel` ends bit-identical to enqueueing the
 * kernels one by one: the colour where a stage hits, (0, 0, 0, 255) elsewhere.
 * Stages.  assign 4: the brute-force mesh (t_pos .. t_mcolor, t_size triangles).  assign 7: the molecule (s_atoms, s_slab_size) and / or the mesh
 * (t_pos, t_normal, t_slab_size; A07's kernels bind t_mindex / t_mcolor / s_mindex / s_mcolor but never read them: they may be NULL), both in grids of
 * n_slabs cells per axis over `bounds`; with both set the mesh is traced after the molecule, from the maxt the molecule left, as computeBoth's
 * second kernel does (the page gives each model's kernel the model's own box; here both grids span the one `bounds`).  A stage is asked for by its first buffer (t_pos, s_atoms) being non-NULL.
 * `rays`, optional: the finished ray per pixel (o, d, mint, final maxt: the 40 bytes of the 48 the kernels write), as the launches leave it.
 * Checks are those of mirt_enqueue on the same kernels: MIRT_E_RANGE for a buffer smaller than the launch touches (pixel, rays, a cell table shorter
 * than n_slabs^3 + 1, primitive arrays shorter than the table says), MIRT_E_DATA for a table that fails validation; MIRT_E_ARG for assign other than
 * 4 or 7, a molecule with assign 4, no stage, or a camera block whose image size is not width x height.  Nothing is written when a check fails.
 * Inside mirt_capture_begin / mirt_capture_end under the rule of mirt_render_pass: run it once before recording it. */
typedef struct mirt_frame_desc {
    uint32_t struct_size;           /* sizeof(mirt_frame_desc)                                      */
    uint32_t assign;                /* 4 or 7                                                       */
    uint32_t width, height;
    float cam[16];                  /* Camera.toFloat32Array (A04 code.js / A07 code.js:73-81)      */
    float bounds[8];                /* assign 7: (min,1,max,1) of the model(s); ignored for 4       */
    uint32_t t_size;                /* mesh: triangles (assign 4), informative for assign 7         */
    uint32_t s_size;                /* molecule: atoms, informative                                 */
    mirt_buf *t_pos, *t_normal, *t_mindex, *t_mcolor;   /* mesh, or t_pos NULL                      */
    mirt_buf *s_atoms, *s_mindex, *s_mcolor;            /* molecule, or s_atoms NULL                */
    uint32_t n_slabs;               /* assign 7: cells per axis of both grids                       */
    uint32_t reserved;
    mirt_buf* t_slab_size;          /* assign 7 mesh: uint[n_slabs^3 + 1]                           */
    mirt_buf* s_slab_size;          /* assign 7 molecule: uint[n_slabs^3 + 1]                       */
    mirt_buf* pixel;                /* uchar4 per pixel                                             */
    mirt_buf* rays;                 /* optional: 48 bytes per pixel                                 */
} mirt_frame_desc;
MIRT_API int mirt_render_frame(mirt_ctx* ctx, const mirt_frame_desc* desc);

/* ---- extension: the anti-aliased frame, aa x aa samples a pixel in one launch ----------------------
 * `desc` is exactly mirt_render_frame's descriptor of the aliased W x H frame (width = W, height = H, cam[14] = W, cam[15] = H); `aa` is the number of
 * samples per axis, 1 to 4.  `pixel` receives W x H pixels; the aa*W x aa*H samples never reach memory.  The camera window (cam[12], cam[13]) is given
 * in scene space, so a camera block that differs only in its column and row counts shows the same frustum on a finer lattice.  Operation by operation:
 *   - the FINE frame F is what mirt_render_frame writes into `pixel` for the same descriptor with width = aa*W, height = aa*H,
 *     cam[14] = (float)(aa*W), cam[15] = (float)(aa*H) and everything else bit-identical, cam[12] and cam[13] included;
 *   - output pixel (x, y), per channel c of R, G, B:  S = the integer sum of byte c of F at (aa*x + i, aa*y + j) over i, j = 0 .. aa-1, and
 *     out.c = (S + floor(aa*aa / 2)) div (aa*aa): the average, halves rounded up.  The sums are integers, so their order is free.  Alpha is 255.
 *   - a sample that misses is F's black (0, 0, 0) and counts like any other;
 *   - the bytes are averaged as the kernels write them: no gamma is undone or applied and every sample weighs the same (a box filter).
 * aa == 1 is mirt_render_frame, `rays` allowed.  MIRT_E_ARG: aa of 0 or above 4; aa > 1 with `rays` non-NULL (a pixel has no one ray); aa*width or
 * aa*height above 65535.  Every other check is mirt_render_frame's own, on the same descriptor, made before anything is queued: nothing is written
 * when one fails.  Assign 4 and 7; the molecule, the mesh and both.  Capture: mirt_render_frame's rule.  The frame fusion of the pages' enqueue
 * streams (below) is untouched: the pages have no such mode.
 * MIRT_ABI_VERSION is unchanged: a host detects the entry point by its symbol. */
MIRT_API int mirt_render_frame_aa(mirt_ctx* ctx, const mirt_frame_desc* desc, uint32_t aa);

/* Command-stream fusion of the frame dialects: the Assign04 / Assign07 pages' own enqueue stream at the one-launch frame's speed, with no change to
 * the host.  A separate switch from mirt_ctx_set_fusion (whose levels keep their meaning), off by default; MIRT_FRAME_FUSION=1 in the environment
 * turns it on for every new context.  With it on an "A04:" / "A07:" initTrace enqueue is held back, and so are the enqueues that follow it (at most three);
 * when the held stream IS a frame as the pages issue it -- initTrace then meshTrace (computeTri), initTrace then molTrace (compute), or initTrace,
 * molTrace, meshTrace (computeBoth), every stage over the same pixels, camera block, rays and box, with the initTrace's global size, which covers the
 * image -- it runs as ONE launch of mirt_render_frame.  Anything else is launched enqueue by enqueue, in order, exactly as with the switch off.  The
 * held stream runs at the first command that would flush a held Assign10 pass (see mirt_ctx_set_fusion: buffer read / write / release, another
 * enqueue that does not continue the frame, capture, timers, destroy ...) and also at mirt_finish.
 *   - pixels after the frame are bit-identical to the switch being off; the Ray buffer is NOT written by a fused frame -- it keeps its previous
 *     contents.  The pages never read it (they cannot: they do not know its layout beyond sizeof).
 *   - errors of a held enqueue are reported by the call that flushes it, as for a held pass.
 * mirt_ctx_fused_frames: how many frames of this context ran fused. */
MIRT_API int mirt_ctx_set_frame_fusion(mirt_ctx* ctx, int on);
MIRT_API int mirt_ctx_fused_frames(mirt_ctx* ctx, uint64_t* count);

/* seeds[i] = 1 + (mix32((first_ray + i) ^ 0x9E3779B9 ^ seed_base) mod 2147483646): the
 * reproducible stand-in for the host's Math.random() seeding (A10 code.js:1140-1146). */
MIRT_API int mirt_seed_fill(mirt_ctx* ctx, mirt_buf* seeds, uint64_t first_ray, uint64_t count, uint32_t seed_base);
/* initAcu over a whole buffer (A10 code.js:1078-1099) */
MIRT_API int mirt_zero(mirt_ctx* ctx, mirt_buf* buf);

/* ---- uniform-grid build on the device: splitSphereData / splitTriangleData / splitMeshData (A10 code.js:1554-1772, 899-1041)
 * and Mesh.normalize/scale/translate (code.js:114-169) as a count / scan / stable-sort / gather pipeline in fp64, reproducing
 * the reference's cell order, per-cell input order and its dropped-on-the-max-face quirk bit for bit.  Every output is a
 * new buffer the caller owns (release it) and can bind to a kernel or put in a mirt_grid. ---------------------------------- */
typedef struct mirt_grid_build_desc {
    uint32_t struct_size;
    uint32_t kind;          /* 0: spheres, 4 doubles per primitive (cx, cy, cz, r); 1: triangles, 9 doubles (p0, p1, p2) */
    uint32_t count;         /* primitives */
    uint32_t n_slabs;       /* cells per axis */
    double bounds[6];       /* min x,y,z, max x,y,z of the set (Bounds, lib/utilities.js:389-422) */
    mirt_buf* prims_f64;    /* device buffer of doubles, uploaded with mirt_buf_write */
} mirt_grid_build_desc;
/* ---- mesh ingest on the device: parseMeshJSON (A10 tri/meshDataVersion1.js:12-78) for one (node, mesh) pair of an Assimp-style mesh
 * file: every triangle corner de-indexed, its position through the node's model matrix (gl-matrix vec3.transformMat4 on Float32Array
 * operands: fp32 matrix, double sums, fp32 store) and its normal through the normal matrix (vec3.transformMat3), written as the fp64
 * soups mirt_grid_build / mirt_grid_gather_triangles consume, at corner offset `first_corner`; `bounds6` (6 floats: min xyz, max xyz,
 * initialise to +inf / -inf) is merged with the mesh's TRANSFORMED vertices, all of them (:33-37).  The normal matrix
 * (mat3.normalFromMat4 of the model matrix, nine floats) is per node and computed by the caller.  Synchronises (an index past the
 * vertex array is MIRT_E_DATA).  Bit-identical to the reference host's arrays (tests/test_js_host.py, device vs host ingest). */
typedef struct mirt_mesh_ingest_desc {
    uint32_t struct_size;
    uint32_t n_vertices;        /* entries of positions / normals (3 doubles each) */
    uint32_t n_corners;         /* 3 x triangles of this mesh: indices.length, or n_vertices when un-indexed */
    uint32_t first_corner;      /* where this (node, mesh) pair's corners start in the output soups */
    float model[16];            /* node.modelMatrix narrowed to fp32 (mat4.copy into a Float32Array), column-major */
    float normal_mat[9];        /* mat3.normalFromMat4(model) */
    mirt_buf* positions_f64;    /* mesh.vertexPositions */
    mirt_buf* normals_f64;      /* mesh.vertexNormals */
    mirt_buf* indices_u32;      /* mesh.indices, or NULL */
} mirt_mesh_ingest_desc;
MIRT_API int mirt_mesh_ingest(mirt_ctx* ctx, const mirt_mesh_ingest_desc* d, mirt_buf* pos9_out, mirt_buf* nor9_out, mirt_buf* bounds6);

/* cell_offsets: uint[n^3+1]; order: uint[total], order[slot] = input index of the primitive in that slot */
MIRT_API int mirt_grid_build(mirt_ctx* ctx, const mirt_grid_build_desc* d, mirt_buf** cell_offsets, mirt_buf** order, uint32_t* total);
/* slot arrays from `order`.  Triangles: 3 x float4 per slot (w = pad_w: 0 in A07/A10, 1 for A04's positions), after up to four
 * fp64 per-axis steps (op 0 subtract, 1 multiply, 2 add; vecs = 3 doubles per step) applied in order, then narrowed to fp32.
 * nor_f64 / nor_out may be NULL. */
MIRT_API int mirt_grid_gather_triangles(mirt_ctx* ctx, mirt_buf* order, uint32_t total, mirt_buf* pos_f64, mirt_buf* nor_f64,
                                        uint32_t nsteps, const int32_t* ops, const double* vecs, float pad_w,
                                        mirt_buf** pos_out, mirt_buf** nor_out);
MIRT_API int mirt_grid_gather_spheres(mirt_ctx* ctx, mirt_buf* order, uint32_t total, mirt_buf* sph_f64, mirt_buf** out);   /* float4 (c, r*r) */
MIRT_API int mirt_grid_gather_u32(mirt_ctx* ctx, mirt_buf* order, uint32_t total, mirt_buf* in_u32, mirt_buf** out);       /* material ids */

/* ---- diagnostics: evaluate one primitive of the numerics contract element-wise on the device
 * (op: 0 a/b, 1 sqrt, 2 sin, 3 cos, 4 getRand(seed=bits of a), 5 next LCG state, 6 min, 7 max, 8 fmin, 9 fmax,
 * 10 normalize(a,b,1).x, 11/12 concentric_distort(a,b).x/.y, 13 (int)a, 14 (uint)a, 25 clamp(a,0,b);
 * float3 arguments as three consecutive floats per element: 20 dot, 21 cross (3 outputs), 22 length, 23 distance,
 * 24 normalize (3 outputs), 26 mad(a.x,a.y,a.z), 27 the four contraction shapes a*b+c, a*b-c, c-a*b, a*b+c*a (4 outputs),
 * 28 the optimistic kernel's ray-side guard (csrc/pt_trace.hpp ray_guard) for a ray with origin a and direction b: 1.0 where the guard
 * accepts the ray -- every |b_k| in [2^-40, 2^40], every a_k zero or |a_k| in [2^-30, 2^20] -- and 0.0 where it refuses it).
 * Lets a test compare device bits with AMD's OpenCL library (oracle/probe/builtins.cl) over millions of inputs. ---- */
MIRT_API int mirt_debug_numerics(mirt_ctx* ctx, int op, mirt_buf* a, mirt_buf* b, mirt_buf* out, size_t n);

/* the PREPARED copy the runtime keeps of a triangle position buffer holding `count` triangles (3 x float4 each), built on first use by a pass
 * or frame kernel and rebuilt when the buffer's contents change: `count` records of 48 bytes {p0, n.x}{e1, n.y}{e2, n.z}, one bounding sphere
 * (float4) per 16 records, and -- for at most 96 records -- the candidate sweep's plane list (64-byte aligned; csrc/pt_launch.hpp).  Copies up
 * to `bytes` of it to `out` and reports its size in *total.  For the tests that pin its layout against the CPU restatement. */
MIRT_API int mirt_debug_prepared(mirt_ctx* ctx, mirt_buf* positions, uint32_t count, void* out, size_t bytes, size_t* total);

/* counts mismatches between the shared-reciprocal division forms of pt_numerics.hpp and the compiler's correctly
 * rounded division over `count` generated (n, d) pairs; `out16` receives 16 uint64 (see k_divCheck).
 * mode 0/1/2: random pairs inside the windows; 3: all 2^32 denominators of the reciprocal; 4: every numerator mantissa
 * against the `count` denominator mantissas starting at `seed` (2^23 launches' worth covers all 2^46 pairs); 5: the 9-operation
 * correctly rounded sqrt over all 2^32 bit patterns (out[1] mismatches of cl_sqrt, out[2] / out[3] of the bare core / outside denormals);
 * 6: the fused pass's concentric-map quotient (out[1]) and single-cell exit quotient (out[2]) over `count` operand pairs of their domains */
MIRT_API int mirt_debug_divcheck(mirt_ctx* ctx, int mode, uint64_t seed, uint64_t count, mirt_buf* out16);

/* ---- launch-bound sequences as HIP graphs ------------------------------------------------------
 * The reference's executeRender() is 44+ enqueues per pass (A10 code.js:1806-1854); on a 320x240 canvas at one ray per pixel (the
 * page's defaults, index.html:46, code.js:400) every one of them is a few microseconds of work behind a launch.  Between
 * mirt_capture_begin and mirt_capture_end every mirt_enqueue / mirt_render_pass / mirt_zero / mirt_seed_fill on the context is
 * recorded instead of run; mirt_graph_launch replays the recording with the argument values it was recorded with.  Run the sequence
 * once normally first: whatever needs a host round trip (cell-table validation, triangle preparation, scratch growth) is cached
 * by that run and refused (MIRT_E_ARG) inside a capture, as are mirt_finish, buffer reads / writes and timers.
 * A recording holds raw device pointers.  Every allocation it touched is pinned by identity: mirt_graph_launch returns MIRT_E_HANDLE
 * once one of those buffers has been released, once the context's scratch memory has been reallocated, or once geometry the
 * recording was validated against (cell offsets, triangle positions) has been rewritten -- record the sequence again. */
typedef struct mirt_graph mirt_graph;
MIRT_API int mirt_capture_begin(mirt_ctx* ctx);
MIRT_API int mirt_capture_end(mirt_ctx* ctx, mirt_graph** out);
MIRT_API int mirt_graph_launch(mirt_ctx* ctx, mirt_graph* graph);
MIRT_API int mirt_graph_release(mirt_graph* graph);

/* ---- several devices in one process: row tiles + the one exchange of the path --------------------------------------------
 * The reference is a single-device page (one context, one queue: A10 code.js:582, 592).  Every ray is independent, so a frame
 * shards by pixel rows; ray ids stay global (mirt_pass_desc.row0 / nrows), which makes the frame independent of the tiling.
 * A group is N contexts, one per device, driven from the one host thread: enqueue the tile passes on each context (launches are
 * asynchronous), then mirt_gather assembles the tiles' buffers on the root device.  Transports: RCCL (ncclCommInitAll + one grouped
 * ncclSend / ncclRecv exchange: N - 1 peers, N - 1 distinct xGMI links into the root; librccl is loaded on first use), or plain copies
 * queued on the root's stream (hipMemcpyPeerAsync across devices, a device copy inside one), each ordered after the tile's own stream.
 * MIRT_GATHER_AUTO picks RCCL for N > 1 distinct devices when librccl loads, copies otherwise; _RCCL / _COPY force one (a one-GPU box
 * exercises the RCCL calls with a one-rank communicator).
 * Rehearsal switch: with MIRT_GROUP_ALLOW_REPEATED_DEVICES=1 in the environment mirt_group_create accepts a device listed several
 * times -- N contexts on the devices at hand, so the whole N-tile path runs on a one-GPU box; such a group gathers by copies only. */
typedef struct mirt_group mirt_group;
MIRT_API int mirt_group_create(const int* device_ids, int n, mirt_group** out);
MIRT_API int mirt_group_size(const mirt_group* g);
MIRT_API mirt_ctx* mirt_group_ctx(const mirt_group* g, int index);     /* owned by the group: do not mirt_ctx_destroy it */
MIRT_API int mirt_group_destroy(mirt_group* g);                       /* destroys its contexts and everything created on them */
MIRT_API int mirt_group_finish(mirt_group* g);                        /* queue.finish() on every device */
/* contiguous row tiles whose sizes differ by at most one row (the first height % n_tiles tiles take the extra one) */
MIRT_API void mirt_tile_rows(uint32_t height, uint32_t n_tiles, uint32_t index, uint32_t* row0, uint32_t* nrows);
/* out[sum of tile_bytes[0..i-1] ...] = the first tile_bytes[i] bytes of tiles[i] (a buffer of context i), for every i < n_tiles
 * (n_tiles must equal mirt_group_size); `out` is a buffer of context `root`.  Ordered after the work queued on each context; complete after mirt_finish(root ctx). */
enum { MIRT_GATHER_AUTO = 0, MIRT_GATHER_RCCL = 1, MIRT_GATHER_COPY = 2 };
MIRT_API int mirt_gather(mirt_group* g, mirt_buf* const* tiles, const size_t* tile_bytes, int n_tiles, mirt_buf* out, int root, int transport);
/* What a group can do and what the last gather did.  mirt_group_create asks hipDeviceCanAccessPeer for every pair of distinct devices and enables peer
 * access both ways; mirt_group_peer_access(g, i, j) = 1 when context i's device reads context j's device's memory directly (always 1 for i == j and for
 * contexts that share a device), 0 when the runtime refused -- then a copy between them is staged through host memory by the HIP runtime.
 * mirt_gather_route(g, tile): how the LAST mirt_gather moved that tile -- MIRT_GATHER_AUTO may pick copies without saying so (librccl absent, a
 * rehearsal group), and a staged copy is an order of magnitude slower than a peer one: a first run on N real GPUs is diagnosable from these. */
enum { MIRT_ROUTE_NONE = 0,   /* no gather yet, or an empty tile                                       */
       MIRT_ROUTE_RCCL = 1,   /* ncclSend / ncclRecv                                                    */
       MIRT_ROUTE_PEER = 2,   /* hipMemcpyPeerAsync between devices with peer access enabled (xGMI P2P) */
       MIRT_ROUTE_STAGED = 3, /* hipMemcpyPeerAsync WITHOUT peer access: bounced through host memory    */
       MIRT_ROUTE_LOCAL = 4 };/* the tile already lives on the root's device: a device-local copy      */
MIRT_API int mirt_group_peer_access(const mirt_group* g, int i, int j);
MIRT_API int mirt_gather_route(const mirt_group* g, int tile);

/* ---- the post-process stage in ROW TILES: every context filters and upsamples the rows it rendered, after a halo exchange -------------------
 * Neither mirt_filter_atrous nor mirt_upsample_guided depends on a pixel's absolute row, except at the image's top and bottom edge.
 *   Filter: iteration i reads rows within 2 * 2^i of the row it writes, so rows [row0, row0 + nrows) after n iterations depend on the input rows
 *   within H = 2 * (2^n - 1) of them and on nothing else.  Filtering the window [row0 - H, row0 + nrows + H), clamped to the image, as if it were
 *   an image gives those rows bit for bit: a clamped edge IS the image's edge, and at an edge that is not, the rows that come out wrong are rows
 *   nobody needs.  One row less, at either end, does not (tests/test_post_rows_restatement.py).
 *   Upsampler: high row y reads low rows Y0(y), Y0(y) + 1 and y div factor, the last always one of the first two inside the low image: high rows
 *   [row0, row0 + nrows) need low rows max(0, Y0(row0)) up to min(height / factor, Y0(row0 + nrows - 1) + 2).
 * So the result of the post chain in tiles is defined with no new numerics: the bits of the whole-frame calls, in both libraries.  What moves
 * between devices is the halo rows, and into the root 4 B per pixel (16 more with `filtered` / `upsampled`) instead of the 52 B per pixel of
 * pixel, radiance and both guides.  NOT built: an RCCL transport for the exchange, graph capture of any of these calls.  Like everything with N
 * contexts, none of it has run on N distinct devices: rehearsal groups on one device only.
 *
 * The two windows, one definition for every host (csrc/pt_rows_plan.hpp), beside mirt_tile_rows.  Both write 0, 0 on bad input: no rows, rows
 * outside the image, iterations > MIRT_FILTER_MAX_ITERATIONS, a factor outside 2 .. 4 or one that does not divide height, height above 65535. */
MIRT_API void mirt_filter_window_rows(uint32_t image_height, uint32_t row0, uint32_t nrows, uint32_t iterations, uint32_t* win_row0, uint32_t* win_nrows);
MIRT_API void mirt_upsample_low_rows(uint32_t height, uint32_t factor, uint32_t row0, uint32_t nrows, uint32_t* lo_row0, uint32_t* lo_nrows);
/* mirt_filter_atrous on rows [row0, row0 + nrows) of an image of desc->width x image_height pixels.  The descriptor is read as follows:
 * desc->height is the number of rows the three INPUT buffers hold, image rows [win_row0, win_row0 + desc->height), the window; `filtered` and
 * `pixel` hold nrows rows, image rows [row0, row0 + nrows), and nothing else.  The window lies inside [0, image_height) and contains
 * mirt_filter_window_rows(image_height, row0, nrows, iterations); a larger window is allowed and changes nothing.
 * Result: both outputs equal, bit for bit, rows [row0, row0 + nrows) of what mirt_filter_atrous writes for the whole frame, with either structure
 * flag or neither, iterations 0 .. 5, in both libraries.
 * How: mirt_filter_atrous's kernels, instantiated for a window.  Every iteration's edge test means the window's edge; iteration i of n computes
 * only the rows still needed, the own rows and 2 * (2^n - 2^(i + 1)) around them; the last step (the prepare, for 0 iterations) reads radiance.w
 * and the guides at the window's offset and stores the own rows alone.  Working memory: three float4 per pixel of the WINDOW, in the context's scratch buffer.
 * Checks, all before anything is queued; nothing is written when one fails: those of mirt_filter_atrous (with image_height for the extent), and
 * MIRT_E_ARG for nrows or desc->height 0, rows or a window that reach outside the image, a window that does not contain the rows needed;
 * MIRT_E_RANGE for an input smaller than the window or an output smaller than nrows rows. */
MIRT_API int mirt_filter_atrous_rows(mirt_ctx* ctx, const mirt_filter_desc* desc, uint32_t image_height, uint32_t win_row0, uint32_t row0, uint32_t nrows);
/* mirt_upsample_guided on high rows [row0, row0 + nrows).  desc->width and desc->height are the WHOLE high image and mirt_upsample_guided's checks
 * apply to them unchanged; normal_hits, albedo_depth, upsampled and pixel hold high rows [row0, row0 + nrows) and nothing else; the three low
 * inputs hold low rows [lo_row0, lo_row0 + lo_nrows), a range inside the low image that contains mirt_upsample_low_rows(height, factor, row0,
 * nrows); a larger one is allowed and changes nothing.
 * Result: rows [row0, row0 + nrows) of the whole-frame call, bit for bit, in both libraries.
 * How: the tap geometry is worked on the global row y = row0 + the band's row and the taps are tested against the low IMAGE (0 <= Y < height /
 * factor); the low buffers are indexed at Y - lo_row0.  Tile borders from mirt_tile_rows are not multiples of factor (1080 rows over 8 is 135).
 * Checks as above: those of mirt_upsample_guided, MIRT_E_ARG for the rules of the rows, MIRT_E_RANGE for the buffer sizes of the two extents. */
MIRT_API int mirt_upsample_guided_rows(mirt_ctx* ctx, const mirt_upsample_desc* desc, uint32_t row0, uint32_t nrows, uint32_t lo_row0, uint32_t lo_nrows);
/* THE HALO EXCHANGE.  All arrays have n entries, n = mirt_group_size; rows are row_bytes bytes each (width * 16 for the float4 images).
 * src[i] is a buffer of context i whose first src_nrows[i] rows are image rows from src_row0[i] on: a tile as a pass, mirt_render_guides or
 * mirt_filter_atrous_rows wrote it.  dst[i] is a buffer of context i that ends holding image rows [dst_row0[i], dst_row0[i] + dst_nrows[i]) from
 * its first byte on: every row copied from whichever source owns it, the context's own rows included.  A window may span several owners (tiles
 * can be shorter than the halo).  A NULL src[i] or dst[i] with 0 rows is allowed: a context that owns nothing, or wants nothing.
 * Transport: copies only -- a device copy inside one device, hipMemcpyPeerAsync across devices (mirt_gather's copy transport).
 * Ordering, so that nothing waits in a circle: (1) one event is recorded on every source context's stream; (2) each destination's stream waits for
 * the events of the owners it reads, queues its copies and records an event; (3) each source's stream then waits for the events of the
 * destinations that read it.  So the copies see everything queued on the sources before the call, and a source may overwrite its tile with the
 * next pass without a mirt_finish.  Complete after mirt_finish of the destination's context.
 * Refusals; nothing is queued on any device when one applies.  MIRT_E_ARG: a null array, n that is not the group's size, row_bytes 0 or not a
 * multiple of 4, two sources that own the same row, a wanted row that nobody owns, a destination whose bytes meet a source's or another
 * destination's, a call while any context is capturing.  MIRT_E_HANDLE: a bad group, a buffer that is not live or not its context's (NULL with
 * rows included).  MIRT_E_RANGE: a buffer shorter than its rows.  Held command streams are flushed first, as mirt_gather does. */
MIRT_API int mirt_exchange_rows(mirt_group* g, mirt_buf* const* src, const uint32_t* src_row0, const uint32_t* src_nrows, mirt_buf* const* dst,
                                const uint32_t* dst_row0, const uint32_t* dst_nrows, int n, size_t row_bytes);

/* ---- measurement: HIP events on the context's stream ---------------------------------- */
MIRT_API int mirt_timer_start(mirt_ctx* ctx);
MIRT_API int mirt_timer_stop_ms(mirt_ctx* ctx, float* ms);   /* synchronises */
/* per-kernel events inside mirt_render_pass: duration of the fused pass kernel and of the resolve
 * (copyToPixel) kernel of the most recent profiled pass, on the stream they were launched on */
MIRT_API int mirt_ctx_set_profiling(mirt_ctx* ctx, int on);
MIRT_API int mirt_pass_timing(mirt_ctx* ctx, float* fused_ms, float* resolve_ms);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_H */
