/*
 * rt.h — C-ABI of the MI355X per-pixel ray tracer (libopenglraytracer_amd.so).
 *
 * Drop-in for the reference's frame-driver -> compute-shader boundary:
 *
 *   reference (OpenGLRaytracer/main.cpp)          this ABI
 *   ------------------------------------------    ------------------------------
 *   :203 createShaderProgram("raytrace_compute")  rt_create()           (once)
 *   :129-159 RGBA8 W x H texture (host-owned)     caller-owned float4 buffer
 *   raytrace_compute.glsl:74-321 scene consts     rt_scene_create()     (per scene/time)
 *   :213 get_current_time(), :226 uniform time    `time` argument
 *   :223 glBindImageTexture + :235 glDispatch     rt_render()
 *   :238 glFinish                                 rt_render() with stream == NULL
 *
 * All structs are plain C, float32, no padding surprises (4-byte members
 * only). Every entry point returns RT_OK (0) or a negative RT_ERR_* code and
 * never throws across the boundary; rt_last_error() returns a thread-local
 * message for the last failure on the calling thread.
 *
 * Output layout (identical to the reference image, raytrace_compute.glsl:404):
 * row-major, row 0 = y 0 (GL's bottom row), pixel (x, y) at index y*W + x,
 * 4 floats (r, g, b, 0) per pixel, unclamped (the shipped RGBA8 surface
 * clamps; rt_pack_rgba8 reproduces that).
 */
#ifndef OPENGLRAYTRACER_AMD_RT_H
#define OPENGLRAYTRACER_AMD_RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_ERR_INVALID (-1)     /* bad argument */
#define RT_ERR_HIP (-2)         /* HIP runtime error */
#define RT_ERR_NOMEM (-3)       /* allocation failed */
#define RT_ERR_UNSUPPORTED (-4) /* e.g. max_depth above RT_MAX_DEPTH */
#define RT_ERR_NO_DEVICE (-5)   /* no GPU / bad device index */

/* Deepest recursion compiled into the kernel. The reference's stack machine
 * (raytrace_compute.glsl:873-874,1077-1101) holds 100 elements and gives up
 * after 10000 steps; with at most 2^(D+1)-1 traced rays of 6 steps each the
 * step guard cannot trigger for D <= 9, so results are exact up to here. */
#define RT_MAX_DEPTH 9

/* raytrace_compute.glsl:56-69 Material */
typedef struct rt_material {
    float ambient[4];
    float diffuse[4];
    float specular[4];
    float shininess;
    float emissive[4];
    float reflectivity;
    float transparency;
    float refraction_index;
} rt_material;

/* raytrace_compute.glsl:244-258 Object (Box :166-170, Sphere :172-175).
 * Type test exactly as get_closest_collision (:749-771): a box when
 * box_mins/box_maxs are not both (0,0,0) (null_box, :178); otherwise a sphere
 * when radius != -1 (null_sphere, :179); otherwise skipped. */
typedef struct rt_object {
    float box_mins[3];
    float box_maxs[3];
    float radius;
    float position[3];
    float angles[3]; /* pitch, yaw, roll in degrees (:254) */
    int32_t material; /* index into the scene's material table */
} rt_object;

/* raytrace_compute.glsl:190-196 Light (point light, Phong terms) */
typedef struct rt_light {
    float position[3];
    float ambient[4];
    float diffuse[4];
    float specular[4];
} rt_light;

/* raytrace_compute.glsl:36-50 Camera */
typedef struct rt_camera {
    float position[3];
    float angles[3]; /* pitch, yaw, roll in degrees */
    float v_fov;     /* degrees */
    float aspect;    /* the reference fixes 16/9 whatever W/H is (:363) */
    float near_plane;
    float far_plane;
} rt_camera;

/* The per-frame camera constants the kernel consumes: the column-major
 * inverse(proj * view) that unprojects NDC (:383) and the ray origin, the
 * camera position (:391). rt_make_view(NULL, time) — the reference's orbit
 * camera, and what rt_render(cam = NULL) uses — evaluates them in float32
 * exactly as the reference's GL (llvmpipe) does (rt_camera.cpp; bit-exact vs
 * tests/golden/camera_llvmpipe.npz); an explicit rt_camera, which the
 * reference does not have, is evaluated in float64 and rounded once to
 * float32. Callers may also supply their own (e.g. a value another renderer
 * computed). */
typedef struct rt_view {
    float unprojection[16];
    float origin[3];
} rt_view;

typedef struct rt_context rt_context; /* one per device; not thread-safe */
typedef struct rt_scene rt_scene;     /* device-resident, precomputed scene */

/* ---- reference scene / camera (host functions, no GPU) --------------- */

/* The 7 materials of raytrace_compute.glsl:74-157, in this order:
 * material1, material2, red_glass, green_glass, blue_glass, mirror, wall. */
#define RT_MAT_MATERIAL1 0
#define RT_MAT_MATERIAL2 1
#define RT_MAT_RED_GLASS 2
#define RT_MAT_GREEN_GLASS 3
#define RT_MAT_BLUE_GLASS 4
#define RT_MAT_MIRROR 5
#define RT_MAT_WALL 6
#define RT_REFERENCE_MATERIALS 7
#define RT_REFERENCE_LIGHTS 3
#define RT_REFERENCE_OBJECTS 5

int rt_reference_materials(rt_material out[RT_REFERENCE_MATERIALS]);
/* raytrace_compute.glsl:199-224 */
int rt_reference_lights(rt_light out[RT_REFERENCE_LIGHTS]);
/* raytrace_compute.glsl:236-237,261-321: the shipped, time-animated scene. */
int rt_reference_objects(float time, rt_object out[RT_REFERENCE_OBJECTS]);
/* raytrace_compute.glsl:334-364: the orbiting camera at `time`. */
int rt_reference_camera(float time, rt_camera *out);
/* Benchmark scenes: object 0 is the reference room box
 * (+-11, wall material); then n_spheres seeded spheres (splitmix64 stream,
 * centre U([-8,8]x[-8,8]x[-4,4]), radius U(0.3,1.2), materials cycling
 * material1, material2, red_glass, green_glass, blue_glass, mirror).
 * `out` holds n_spheres + 1 objects. */
int rt_bench_objects(int n_spheres, uint64_t seed, rt_object *out);

/* cam == NULL: the reference orbit camera at `time`. */
int rt_make_view(const rt_camera *cam, float time, rt_view *out);

/* ---- scenes as functions of `time` (host functions, no GPU) ------------
 * The reference moves its objects inside the shader from the one uniform
 * `time` (raytrace_compute.glsl:236-237, :261-321). Here that motion is
 * described per object by scalar channels; a zero-initialised rt_object_anim
 * means "static", so an existing scene describes itself. Every expression is
 * float32, in exactly the written operation order, with no fused
 * multiply-add; sin is the reference GL's run-time sin (gallivm's polynomial,
 * rt_glmath.h). The forms are kept apart on purpose: 0 + x and x differ for
 * x = -0. `k` is the folded constant the reference's GL forms (time_scale * K
 * = 0.4f * K, :236).
 * Range of `time`: the run-time sin / cos truncate |angle in radians| * 4/pi
 * to an int, so every sin argument time * k, and every angle (degrees times
 * pi / 180), must stay below 2^31 * pi / 4 in magnitude; beyond that host and
 * device differ. */
#define RT_ANIM_NONE        0  /* the base object's value, unchanged            */
#define RT_ANIM_RATE        1  /* time * k                                      */
#define RT_ANIM_RATE_OFFSET 2  /* c + time * k                                  */
#define RT_ANIM_SIN         3  /* sin(time * k) * a                             */
#define RT_ANIM_SIN_OFFSET  4  /* a * sin(time * k) + c                         */
typedef struct rt_anim_channel { int32_t kind; float a, k, c; } rt_anim_channel;
typedef struct rt_object_anim {
    rt_anim_channel scale;        /* multiplies box_mins and box_maxs componentwise */
    rt_anim_channel position[3];  /* replaces position[i]                           */
    rt_anim_channel angles[3];    /* replaces angles[i] (degrees)                   */
} rt_object_anim;
/* The shipped scene's rules (:261-321) in this form: base[] are its objects
 * with the animated fields at their time-0 values, anim[] their channels. */
int rt_reference_animation(rt_object base[RT_REFERENCE_OBJECTS], rt_object_anim anim[RT_REFERENCE_OBJECTS]);
/* out[i] = base[i] with its channels evaluated at `time` (out may be base).
 * For rt_reference_animation the result equals rt_reference_objects(time)
 * byte for byte. An object's kind (box, sphere or null) is the one its BASE
 * has: the animated entry points below lay the scene out once, from the base
 * objects, so a scale channel that passes through 0 does not turn a box into
 * a sphere there (rt_scene_create of this function's output would). */
int rt_animate_objects(const rt_object *base, const rt_object_anim *anim, int n_objs, float time, rt_object *out);
/* The same with a radius channel per object beside the description (a sphere
 * has one field rt_object_anim cannot express): radius[i], n_objs entries in
 * the five forms above, replaces out[i].radius. radius == NULL: no radius
 * moves, and the result equals rt_animate_objects byte for byte. The kind rule
 * above holds for the radius too: on the animated entry points a radius
 * channel that passes through -1 does not turn a sphere into a null object
 * (there it is a sphere of radius 1, as any negative radius r other than -1
 * is a sphere of radius |r|); rt_scene_create of this function's output would
 * make that change. */
int rt_animate_objects2(const rt_object *base, const rt_object_anim *anim, const rt_anim_channel *radius, int n_objs,
                        float time, rt_object *out);

/* The transforms a box object is intersected with, as the reference's GL
 * evaluates them per ray (raytrace_compute.glsl:650-652, :718, replacing
 * calc_transform_matrix / inverse / transpose(inverse(mat3(.)))):
 * local_to_world and world_to_local (column-major 4x4, m[col][row] at
 * col * 4 + row) and the normal matrix (column-major 3x3). The scene builder
 * stores exactly these; exposed for tests and tools. */
int rt_object_transforms(const rt_object *obj, float l2w[16], float w2l[16], float nrm[9]);

/* Scene description input: the content the reference
 * compiles into its shader (materials :74-157, lights :199-224, the animated
 * objects :261-321 at `time`, the camera :334-364) read from JSON text —
 * format in openglraytracer_amd/csrc/rt_scene_json.cpp. Fills the caller's
 * arrays (capacities max_*; n_* = entries written); *has_camera = 1 when the
 * text sets a camera (written to *cam, which may be NULL), else 0 (use the
 * reference orbit camera). Host only; RT_ERR_INVALID with a message naming
 * the problem (and the byte offset of a syntax error). */
int rt_scene_desc_parse(const char *json, float time, rt_object *objs, int max_objs, int *n_objs,
                        rt_material *mats, int max_mats, int *n_mats, rt_light *lights, int max_lights,
                        int *n_lights, rt_camera *cam, int *has_camera);

/* ---- device API ------------------------------------------------------ */
int rt_create(int device, rt_context **out);
void rt_destroy(rt_context *ctx);

/* Copies and precomputes (transforms, inverse transforms, normal matrices)
 * the scene and uploads it to the context's device. Arrays are host memory
 * and may be freed after the call. n_objs <= RT_MAX_OBJECTS.
 * Host cost (make -C openglraytracer_amd/csrc scene-build-time, 8 host
 * threads): about 2-5 ms up to 256 spheres. A scene of 33-256 spheres also
 * gets origin-sphere candidate lists for depth >= 2 renders (RT_OPT_ORIGIN_
 * LISTS; 12.6 MB and about 30 ms at 256 spheres): they are built and
 * appended to the device copy by the first render that reads them, never by
 * create or update, and are not kept on the host.
 * Stream order: create, update and destroy run on the context's stream, a
 * blocking HIP stream (see rt_render): their uploads and stream-ordered
 * frees are ordered after work queued earlier on the device's null stream
 * (torch's default stream), and null-stream work queued later waits for
 * them; create and update return only after their upload is complete. */
#define RT_MAX_OBJECTS 1024
#define RT_MAX_LIGHTS 16
#define RT_MAX_MATERIALS 256
int rt_scene_create(rt_context *ctx, const rt_object *objs, int n_objs, const rt_material *mats,
                    int n_mats, const rt_light *lights, int n_lights, rt_scene **out);
/* Frees the scene's device memory in stream order behind every render that
 * reads it — on the context's stream and on any caller stream (an event per
 * stream is recorded at each render, for up to 8 distinct caller streams);
 * no device-wide synchronisation, except when the scene was rendered on more
 * than 8 distinct caller streams (or an event wait fails): then it waits for
 * the whole device before freeing. rt_scene_update waits the same way. */
void rt_scene_destroy(rt_scene *scene);
/* Replace the scene's contents in place (an animated frame: the reference
 * recomputes its objects from `time` every frame, raytrace_compute.glsl:
 * 277-307); reallocates only if the new scene is larger. Waits (on the host)
 * for the renders queued that read the scene, on any stream. The per-frame
 * host cost is rt_scene_create's build (about 2-5 ms up to 256 spheres, tens
 * of microseconds for the shipped scene) plus the upload; a deep render of
 * the new contents rebuilds the origin-sphere lists once. */
int rt_scene_update(rt_context *ctx, rt_scene *scene, const rt_object *objs, int n_objs, const rt_material *mats,
                    int n_mats, const rt_light *lights, int n_lights);

/* Render rows [row_begin, row_end) of a width x height frame.
 *  cam        NULL = the reference orbit camera at `time` (main(), :334-364).
 *  out        (row_end-row_begin)*width*4 floats; device memory of this
 *             context's GPU if out_is_device, else host memory.
 *  hip_stream hipStream_t; NULL = the context's own stream and the call
 *             returns after the frame is complete (the reference's glFinish,
 *             main.cpp:238). That stream is a blocking HIP stream: the
 *             render starts after all work queued earlier on the device's
 *             null stream (torch's default stream, e.g. a fill of `out`), as
 *             glDispatchCompute follows the earlier commands of its context
 *             (main.cpp:220-238). A non-NULL stream makes the call
 *             asynchronous and ordered only on that stream (out_is_device
 *             must then be 1). Every render entry point below treats
 *             hip_stream the same way.
 * No allocation happens here after the first call at a given size. */
int rt_render(rt_context *ctx, const rt_scene *scene, const rt_camera *cam, float time, int width,
              int height, int max_depth, int row_begin, int row_end, float *out, int out_is_device,
              void *hip_stream);

/* Same, with explicit frame constants. */
int rt_render_view(rt_context *ctx, const rt_scene *scene, const rt_view *view, int width, int height,
                   int max_depth, int row_begin, int row_end, float *out, int out_is_device,
                   void *hip_stream);

/* Row-block interleaved shard for multi-GPU frames: renders the rows r of the
 * frame with (r / block_rows) % n_shards == shard, in increasing order, packed
 * densely into out_device (rt_shard_rows() rows of width*4 floats). */
int rt_shard_rows(int height, int block_rows, int n_shards, int shard);
int rt_render_shard(rt_context *ctx, const rt_scene *scene, const rt_view *view, int width,
                    int height, int max_depth, int block_rows, int n_shards, int shard,
                    float *out_device, void *hip_stream);

/* Several frames in one launch (the reference's frame loop, main.cpp:81-86,
 * batched): views[k] renders into out_device + k * rows * width * 4 floats,
 * where rows = height, or rt_shard_rows(...) when n_shards > 1 (each frame
 * then gets this shard's interleaved row blocks). The scene is shared. Up to
 * 8 views travel in the kernel arguments; 9..RT_MAX_BATCH views of a
 * max_depth 0 or 1 frame go through a device buffer of the context (one
 * launch). Deeper frames run as even launches of as many views as one
 * launch holds beside the scene in GPU local memory (1..8, by the scene's
 * size: 7 for 64 spheres, 1 for 256). */
#define RT_MAX_BATCH 256
/* The number of kernel launches rt_render_batch makes for n_views views of
 * this scene at max_depth (1 up to RT_MAX_BATCH views at depth 0-1; deep
 * batches: ceil(n_views / views per queued launch)), or a negative RT_ERR_*.
 * No GPU work; for callers that time or size per launch. */
int rt_batch_launches(rt_context *ctx, const rt_scene *scene, int n_views, int max_depth);
int rt_render_batch(rt_context *ctx, const rt_scene *scene, const rt_view *views, int n_views, int width,
                    int height, int max_depth, int block_rows, int n_shards, int shard, float *out_device,
                    void *hip_stream);

/* Animated frames in one launch (the reference's frame loop, main.cpp:81-86,
 * where the shipped scene moves with `time`, raytrace_compute.glsl:277-307):
 * as rt_render_batch, but views[k] renders scenes[k]. Every scene must have
 * scene 0's layout — the same object kinds in the same order and the same
 * material and light counts (e.g. rt_reference_objects at successive times,
 * each built with rt_scene_create). */
int rt_render_batch_scenes(rt_context *ctx, const rt_scene *const *scenes, const rt_view *views, int n_views,
                           int width, int height, int max_depth, int block_rows, int n_shards, int shard,
                           float *out_device, void *hip_stream);

/* ---- device-side animation ---------------------------------------------
 * An animated scene: the base objects and their channels, resident on the
 * device. A render at `time` runs an animate kernel on the call's stream
 * that evaluates the channels and rewrites the time-dependent parts of the
 * scene (the boxes' transforms and their culling data; with rt_anim_create2
 * the moving spheres and theirs), then the existing
 * render: no host rebuild, no upload and no host synchronisation per frame
 * (the reference: one uniform, raytrace_compute.glsl:236-237, main.cpp:226).
 * The frame is bit-identical to rt_scene_update(rt_animate_objects(time)) —
 * rt_animate_objects2 with radius channels — followed by the corresponding
 * existing render call.
 *
 * rt_anim_create supports channels on box objects only: an animated sphere
 * (or null object) is refused with RT_ERR_UNSUPPORTED. Spheres may be present
 * and static, in any number.
 * rt_anim_create2 takes a radius channel per object as well (radius, n_objs
 * entries or NULL, as rt_animate_objects2) and moves spheres too: a sphere is
 * moving when a position channel or its radius channel is not RT_ANIM_NONE.
 * The animate kernel then also rewrites the moving spheres' records, refits
 * the bounds of the sphere BVH (its topology is built once, from the base
 * objects), and rewrites their shadow cones and their bits in the shadow
 * direction masks. Angle and scale channels on a sphere are accepted and
 * evaluated by rt_animate_objects2; the render never reads them. An object's
 * kind is its base's (see rt_animate_objects2). Limits: a scene with a moving
 * sphere holds at most 32 spheres in all (larger scenes carry wide masks,
 * candidate lists and origin-sphere lists, which are not rebuilt on the
 * device): RT_ERR_UNSUPPORTED otherwise; a moving sphere's base position and
 * radius and its channels' a, k, c must be finite (RT_ERR_INVALID); channels
 * on null objects stay refused. With radius == NULL and no channel on a
 * sphere it behaves as rt_anim_create.
 * A scene with a RATE / RATE_OFFSET channel on a position, on the scale or on
 * a radius is laid out for |time| <= 1e4 (its culling margins grow with the
 * farthest the objects can get); a render outside that range returns
 * RT_ERR_UNSUPPORTED. `time` must also respect the sin /
 * cos range above. A scene of 33-256 spheres gets its origin-sphere lists at
 * creation, in each of the max_frames frame slots.
 *
 * max_frames (1..RT_MAX_BATCH): the frames that may be in flight at once,
 * each in a slot of its own; a call takes the next slot(s) and, when a slot
 * was last read on another stream, waits for that on the device
 * (hipStreamWaitEvent), never on the host. RT_ERR_INVALID for a NULL
 * pointer, a channel kind outside RT_ANIM_*, max_frames out of range, or
 * (rt_render_batch_animated) n_views > max_frames.
 * rt_last_kernel_ms after these calls covers the render launch or launches
 * only, not the animate launch. An rt_anim that outlives its context is
 * still destroyed safely (synchronously), like a scene. */
typedef struct rt_anim rt_anim;
int rt_anim_create(rt_context *ctx, const rt_object *base, const rt_object_anim *anim, int n_objs,
                   const rt_material *mats, int n_mats, const rt_light *lights, int n_lights, int max_frames,
                   rt_anim **out);
int rt_anim_create2(rt_context *ctx, const rt_object *base, const rt_object_anim *anim, const rt_anim_channel *radius,
                    int n_objs, const rt_material *mats, int n_mats, const rt_light *lights, int n_lights,
                    int max_frames, rt_anim **out);
void rt_anim_destroy(rt_anim *anim);
/* rt_render with the objects at `time` too: cam NULL = the orbit camera at `time`. */
int rt_render_animated(rt_context *ctx, rt_anim *anim, const rt_camera *cam, float time, int width, int height,
                       int max_depth, int row_begin, int row_end, float *out, int out_is_device, void *hip_stream);
/* rt_render_batch_scenes without the scenes: frame k shows the objects at
 * times[k] through views[k] (views NULL: the orbit camera at times[k]). */
int rt_render_batch_animated(rt_context *ctx, rt_anim *anim, const rt_view *views, const float *times, int n_views,
                             int width, int height, int max_depth, int block_rows, int n_shards, int shard,
                             float *out_device, void *hip_stream);

/* Monte-Carlo extension (the reference has one
 * ray per pixel): adds, for every pixel of rows [row_begin, row_end), the sum
 * of samples [sample_offset, sample_offset + spp) — in sample order — to
 * accum_device (float4 per pixel, caller-zeroed, device memory). Sample s of
 * pixel (x, y) is the reference ray through NDC ((x - W/2 + jx) / (W/2),
 * (y - H/2 + jy) / (H/2)) with (jx, jy) in [0, 1)^2 from a counter-based hash
 * of (seed, s, y*W + x) when jitter != 0, else (0, 0) (then every sample
 * equals the reference frame). With hip_stream NULL a zero fill queued on
 * the null stream (torch's default stream) is complete before the
 * accumulation reads the buffer. The mean is accum / total samples. Disjoint
 * sample ranges on several GPUs sum (RCCL all-reduce) to the same estimate
 * up to float re-association. */
int rt_render_accumulate(rt_context *ctx, const rt_scene *scene, const rt_view *view, int width, int height,
                         int max_depth, int spp, int sample_offset, uint32_t seed, int jitter, int row_begin,
                         int row_end, float *accum_device, void *hip_stream);

/* ---- adaptive anti-aliasing ----------------------------------------------
 * Whitted's scheme: one sample per pixel, then supersampling only where the
 * colour changes. The frame is rt_render's (width x height float4, row 0 =
 * GL's bottom row), whole frames only: no row ranges, no shards.
 *  1. The base frame B is rt_render_view of the whole frame at max_depth.
 *  2. Pixel p is flagged iff some 4-neighbour q inside the frame — (x+-1, y),
 *     (x, y+-1) — has max over c in {r, g, b} of |B[p][c] - B[q][c]| >
 *     threshold. float32 throughout; the maximum is IEEE maxNum, so a channel
 *     whose difference is NaN drops out and a NaN difference never flags; an
 *     infinite one does (for a threshold below +inf). Both sides of an edge
 *     are flagged; a 1 x 1 frame flags nothing; threshold +inf flags nothing
 *     and a negative one every pixel that has a neighbour.
 *  3. An unflagged pixel keeps B[p]. A flagged one becomes A[p] / (float)spp,
 *     componentwise IEEE division (alpha stays 0), where A[p] is exactly what
 *     rt_render_accumulate(spp, sample_offset 0, seed, jitter 1) leaves for
 *     the pixel in a zeroed accumulator: the base sample is replaced, not
 *     averaged in.
 * `refined`, optional: one byte per pixel, 1 = flagged; device or host memory
 * as `out` is. out_is_device and hip_stream are rt_render_view's (a non-NULL
 * stream: asynchronous, device memory only). On the device: the base render
 * (whatever kernel rt_render_view would pick), one edge kernel, one refine
 * launch over the flagged pixels, all on the call's stream, nothing waited for
 * or allocated in between after the first call at a size. The scratch
 * (masks, live-tile list, counters) is the context's: a call on another stream
 * waits on the device for the previous call's use of it.
 * Errors: RT_ERR_INVALID for a NULL context ("null context ..."), scene, view
 * or out, spp < 1, a NaN threshold, a bad size; RT_ERR_UNSUPPORTED when
 * RT_OPT_OUTPUT is not RT_OUTPUT_RGBA32F, or for max_depth outside
 * [0, RT_MAX_DEPTH]. RT_OPT_CULLING applies and leaves the output identical.
 * With RT_OPT_TIMING, rt_last_kernel_ms covers the three launches; the
 * rt_debug_last_* hooks keep reporting the base render. */
int rt_render_aa_view(rt_context *ctx, const rt_scene *scene, const rt_view *view, int width, int height,
                      int max_depth, int spp, uint32_t seed, float threshold, float *out, uint8_t *refined,
                      int out_is_device, void *hip_stream);
/* cam == NULL: the reference orbit camera at `time`. */
int rt_render_aa(rt_context *ctx, const rt_scene *scene, const rt_camera *cam, float time, int width, int height,
                 int max_depth, int spp, uint32_t seed, float threshold, float *out, uint8_t *refined,
                 int out_is_device, void *hip_stream);
/* Waits for the context's last anti-aliased render and returns its flagged
 * pixels and its wave tiles (the kernels' 8 x 8 pixel units, aligned at
 * multiples of 8) with a flagged pixel; either may be NULL. For tools and
 * tests. RT_ERR_INVALID before the first such render. */
int rt_aa_last_counts(rt_context *ctx, int64_t *pixels, int64_t *wave_tiles);
/* The criterion itself on the host (no GPU, no context): step 2 over a frame
 * in host memory. refined: one byte per pixel; tile_masks: one 64-bit word
 * per wave tile, row-major ((width + 7) / 8 per row), bit l = pixel
 * (8 wx + l % 8, 8 wy + l / 8), bits of pixels outside the frame 0. Either
 * may be NULL, not both. The same text as the edge kernel evaluates. */
int rt_aa_edge_mask(const float *rgba32f, int width, int height, float threshold, uint8_t *refined,
                    uint64_t *tile_masks);

/* ---- primary-hit buffers and pixel picking ------------------------------
 * What the kernel finds on the way to a pixel's colour, instead of the
 * colour: per pixel, the object its camera ray hits first
 * (get_closest_collision, raytrace_compute.glsl:738-782), the collision's
 * normal and world position, and which lights are occluded from there
 * (the shadow ray of :807-819). For picking, for depth and normal guides of a
 * denoiser over rt_render_accumulate's means, and for debugging a colour.
 *
 * Layout: rt_render's — row-major, row 0 = GL's bottom row, rows
 * [row_begin, row_end), pixel (x, y) at (y - row_begin) * width + x. Three
 * planes, each optional (NULL; not all three): `hits`, one rt_hit per pixel;
 * `normals` and `points`, 4 floats per pixel (x, y, z, 0), (0, 0, 0, 0) for a
 * miss. Every pixel of the row range is written, misses included.
 * The shadow bits cover every light: also one without diffuse and specular
 * colour, whose shadow ray a colour render never casts because it cannot
 * change the colour. With flags = 0 no shadow ray is cast and shadow is 0.
 * RT_OPT_OUTPUT does not apply (the records' formats are fixed);
 * RT_OPT_CULLING applies and leaves the output identical; no other context
 * option changes it. out_is_device, hip_stream and the errors are
 * rt_render_view's (RT_ERR_INVALID for a NULL pointer, a bad size or row
 * range, all three planes NULL, or an unknown flag bit); host planes go
 * through a grow-only device buffer of the context, so no allocation happens
 * after the first call at a given size. With RT_OPT_TIMING,
 * rt_last_kernel_ms covers the hits launch. The hits kernel is not a row of
 * the render kernels' table: rt_debug_last_kernel (and the other
 * rt_debug_last_* hooks) keep reporting the last render launch. */
typedef struct rt_hit {      /* 16 bytes per pixel */
    int32_t  object;         /* index into the scene's objs[], -1 = the ray hit nothing          */
    float    t;              /* get_closest_collision's t (:738-782); 0 for a miss               */
    uint32_t shadow;         /* bit j: light j is occluded from the hit point (:807-819), j < 16 */
    int32_t  material;       /* objs[object].material; -1 for a miss                             */
} rt_hit;
#define RT_HITS_SHADOW 1     /* flags: compute rt_hit.shadow (otherwise 0, and no shadow ray is cast) */
int rt_render_hits_view(rt_context *ctx, const rt_scene *scene, const rt_view *view, int width, int height,
                        int row_begin, int row_end, int flags, rt_hit *hits, float *normals, float *points,
                        int out_is_device, void *hip_stream);
/* cam == NULL: the reference orbit camera at `time`. */
int rt_render_hits(rt_context *ctx, const rt_scene *scene, const rt_camera *cam, float time, int width, int height,
                   int row_begin, int row_end, int flags, rt_hit *hits, float *normals, float *points,
                   int out_is_device, void *hip_stream);
/* rt_render_hits with the objects at `time` too, as rt_render_animated: the
 * animate kernel on the next frame slot, then the hits launch on that slot. */
int rt_render_hits_animated(rt_context *ctx, rt_anim *anim, const rt_camera *cam, float time, int width, int height,
                            int row_begin, int row_end, int flags, rt_hit *hits, float *normals, float *points,
                            int out_is_device, void *hip_stream);
/* The records of one pixel (x, y in the layout's convention: y = 0 is the
 * bottom row) into host memory, synchronously on the context's stream; hit,
 * normal and point may each be NULL, not all three. Renders the pixel's row
 * into the context's buffer and copies 48 bytes back. RT_ERR_INVALID for a
 * pixel outside the frame. */
int rt_pick(rt_context *ctx, const rt_scene *scene, const rt_view *view, int width, int height, int x, int y,
            int flags, rt_hit *hit, float normal[3], float point[3]);

/* ---- ray queries: caller-supplied rays -----------------------------------
 * The same machinery behind a buffer of rays of any origin and direction
 * instead of a pinhole view: a fisheye, orthographic, panoramic or thin-lens
 * camera, a light probe, line-of-sight and range queries, rays continued from
 * a hit that rt_render_hits reported.
 *
 * Ray i is traced as recursive_raytrace (raytrace_compute.glsl:1071-1105)
 * traces a ray with that start and direction, at max_depth 0..RT_MAX_DEPTH.
 * The direction is used as given, not normalised: the reference's rays are
 * unit vectors, and t, the 10000 horizon and the shading assume that.
 * Planes, each optional (NULL; not all four), one 16-byte record per ray:
 * colors[i] = (r, g, b, 0) as rt_render writes a pixel; hits[i], normals[i],
 * points[i] = rt_render_hits' records of the ray's first hit, a miss
 * (-1, 0, 0, -1) and zeros. flags: RT_HITS_SHADOW as for rt_render_hits, dead
 * lights included. max_depth applies to colors only. n_rays = 0 returns RT_OK
 * and does nothing.
 * buffers_are_device covers `rays` and every plane; host buffers go through
 * one grow-only device buffer of the context. hip_stream as in rt_render (a
 * non-NULL stream: asynchronous, device buffers only). At most two launches
 * (colours, hits) on the call's stream. RT_OPT_CULLING applies and leaves the
 * output identical; RT_OPT_OUTPUT does not apply; rt_last_kernel_ms covers the
 * call's launches; the rt_debug_last_* hooks keep reporting the last render.
 * Exact (bit for bit the reference's arithmetic) for every ray whose origin
 * and direction are finite, wherever the origin lies and whatever the
 * direction's length: a wave of 64 consecutive rays that holds an origin more
 * than 1024 units from the world's origin on an axis, or a direction whose
 * squared length differs from 1 by more than 2^-19, is traced without culling
 * (slower, identical). A ray with a non-finite component gives an unspecified
 * record for that ray alone.
 * Errors: RT_ERR_INVALID for a NULL context ("null context ..."), a NULL
 * scene, NULL rays with n_rays > 0, all four planes NULL, n_rays < 0 or
 * > RT_MAX_RAYS, unknown flag bits, a stream with host buffers;
 * RT_ERR_UNSUPPORTED for max_depth outside [0, RT_MAX_DEPTH] when colors is
 * given. */
typedef struct rt_ray {      /* 32 bytes: two 16-byte device loads per lane */
    float origin[3]; float reserved0;   /* reserved*: ignored on input, any value */
    float dir[3];    float reserved1;
} rt_ray;
#define RT_MAX_RAYS (1 << 28)
int rt_trace_rays(rt_context *ctx, const rt_scene *scene, const rt_ray *rays, int64_t n_rays, int max_depth,
                  int flags, float *colors, rt_hit *hits, float *normals, float *points, int buffers_are_device,
                  void *hip_stream);
/* The camera rays of a view in rt_render's pixel order: pixel (x, y) of rows
 * [row_begin, row_end) at (y - row_begin) * width + x, origin = view->origin,
 * direction = exactly what the render kernels compute for the pixel (the same
 * text), reserved words 0. rt_trace_rays of them equals rt_render_view /
 * rt_render_hits_view of the view byte for byte; perturb them for a custom
 * camera. Errors as rt_render_view's (NULL pointer, bad size or row range, a
 * stream with a host buffer: RT_ERR_INVALID). */
int rt_view_rays(rt_context *ctx, const rt_view *view, int width, int height, int row_begin, int row_end,
                 rt_ray *rays, int rays_are_device, void *hip_stream);
/* Occlusion (any-hit) queries: one bit per segment. Ray i is the segment
 * origin + t * dir, 0 < t < 1: dir is the vector to the far end, used as given
 * (the same rt_ray record as rt_trace_rays, so one buffer serves both calls).
 * The segment is occluded iff get_closest_collision
 * (raytrace_compute.glsl:738-782) of that ray returns an object with t < 1.0,
 * the reference's shadow decision (:813-816); that is, iff rt_trace_rays would
 * report hits[i].object >= 0 && hits[i].t < 1.0f, bit for bit, for every ray
 * whose components are finite. It follows that
 *  - a hit at t <= 0 is skipped (:753): a segment that starts exactly on a
 *    surface is not blocked by that surface at t = 0;
 *  - a hit at exactly t == 1.0f does not occlude;
 *  - a segment that starts inside a sphere or box is blocked by the exit hit
 *    when that lies below 1;
 *  - the 10000 horizon plays no part;
 *  - a ray with a non-finite component gets an unspecified answer for that
 *    ray alone.
 * Outputs, either may be NULL, not both: occluded[i], one byte per ray, 1 or
 * 0; words[i / 64] bit i % 64 = ray i, (n_rays + 63) / 64 words, the bits past
 * n_rays in the last word 0. Nothing beyond those counts is written.
 * n_rays = 0 returns RT_OK and does nothing, once the arguments have passed
 * the checks below (n_rays = 0 with both outputs NULL is RT_ERR_INVALID, as
 * rt_trace_rays with no plane). buffers_are_device covers `rays`
 * and both outputs; host buffers go through the context's grow-only ray
 * buffer. hip_stream as in rt_trace_rays (a non-NULL stream: asynchronous,
 * device buffers only). One launch on the call's stream, which stops at a
 * segment's first blocker and searches no further than its far end.
 * RT_OPT_CULLING applies and leaves the output identical (a wave of 64
 * consecutive segments that holds an origin more than 1024 units from the
 * world's origin on an axis, a |dir|^2 outside [2^-64, 2^64], or an origin
 * farther from the scene's spheres than about 512 sqrt(r) units, r the
 * smallest sphere's radius, tests every sphere: slower, identical); RT_OPT_OUTPUT does not apply; rt_last_kernel_ms
 * covers the launch; the rt_debug_last_* hooks keep reporting the last render.
 * Errors: RT_ERR_INVALID for a NULL context ("null context ..."), a NULL
 * scene, a scene of another device, NULL rays with n_rays > 0, both outputs
 * NULL, n_rays < 0 or > RT_MAX_RAYS, a stream with host buffers. */
int rt_occluded(rt_context *ctx, const rt_scene *scene, const rt_ray *rays, int64_t n_rays, uint8_t *occluded,
                uint64_t *words, int buffers_are_device, void *hip_stream);

/* ---- one frame on several GPUs of this process ----
 * The reference renders a frame with one glDispatchCompute(W, H, 1) +
 * glFinish (OpenGLRaytracer/main.cpp:228-238). A multi-GPU group deals the
 * frame's rows in interleaved blocks of block_rows rows to its GPUs (the
 * rt_shard_rows / rt_render_shard layout), every GPU renders its blocks on
 * its context's stream, one gather brings the shards to the first context's
 * GPU (the root) — RCCL point-to-point over xGMI (ncclCommInitAll over the
 * contexts' devices; one context per device) or peer copies — and the root
 * de-interleaves them into the frame. The result is bit-identical to
 * rt_render of the whole frame on one GPU. */
typedef struct rt_multi rt_multi;
#define RT_MULTI_RCCL 0 /* RCCL grouped ncclSend / ncclRecv to the root */
#define RT_MULTI_COPY 1 /* hipMemcpyPeerAsync; also serves contexts that share a device */
/* ctxs[0..n_gpus) stay owned by the caller and must outlive the group. */
int rt_multi_create(int n_gpus, rt_context *const *ctxs, int transport, rt_multi **out);
void rt_multi_destroy(rt_multi *m);
/* scenes[i]: the frame's scene on ctxs[i]'s device (the same content on
 * every device). out: the whole frame in the root context's surface format
 * (RT_OPT_OUTPUT, the same on every context), device memory of the root's
 * GPU if out_is_device, else host memory. Synchronous, like glFinish. */
int rt_render_multi(rt_multi *m, const rt_scene *const *scenes, const rt_camera *cam, float time, int width,
                    int height, int max_depth, int block_rows, float *out, int out_is_device);
int rt_render_multi_view(rt_multi *m, const rt_scene *const *scenes, const rt_view *view, int width, int height,
                         int max_depth, int block_rows, float *out, int out_is_device);
/* Times of the last rt_render_multi: kernel_ms[i] per GPU (-1 when its
 * context's RT_OPT_TIMING is off or it had no rows), the gather (from the
 * moment every shard is complete) and the de-interleave on the root. */
int rt_multi_last_ms(rt_multi *m, float *kernel_ms, float *gather_ms, float *assemble_ms);

/* Context options. RT_OPT_CULLING (default 1): skip spheres that provably
 * cannot be hit (conservative footprints / light cones with margins far
 * above float error) — output is bit-identical either way. */
#define RT_OPT_CULLING 1
/* RT_OPT_TIMING (default 1): record HIP events around every launch for
 * rt_last_kernel_ms. Each event is a marker on the stream; 0 leaves the
 * stream with the kernels alone (back-to-back launches, e.g. a benchmark
 * timing many frames with one event pair of its own). */
#define RT_OPT_TIMING 2
/* RT_OPT_OUTPUT (default RT_OUTPUT_RGBA32F): the surface format renders
 * write. RT_OUTPUT_RGBA8 is the shipped app's GL_RGBA8 texture
 * (OpenGLRaytracer/main.cpp:152-159, :223; raytrace_compute.glsl:404): the
 * kernel packs each pixel in its epilogue — clamp to [0, 1], unorm rounding,
 * exactly rt_pack_rgba8 of the float frame — and stores 4 bytes per pixel, so
 * every `out` buffer then holds width*rows*4 bytes (uint8 r, g, b, a).
 * RT_OUTPUT_RGB32F drops the alpha channel, which is always 0.0 (:404): 3
 * floats per pixel (width*rows*12 bytes), the compact transport form of a
 * float frame (the multi-GPU frame exchange ships 3/4 of the bytes).
 * rt_render_accumulate keeps float4 sums and refuses the other formats. */
#define RT_OPT_OUTPUT 3
#define RT_OUTPUT_RGBA32F 0
#define RT_OUTPUT_RGBA8 1
#define RT_OUTPUT_RGB32F 2
/* RT_OPT_FRAME_CONSTS (default 1): a launch's per-frame constants (every
 * sphere's and box's camera-origin terms and every sphere's pixel footprint,
 * per view) are computed on the host and carried in the kernel arguments when
 * all views' records fit (272 records, at most 256 per view: e.g. 8 views of
 * 16 spheres + 1 box);
 * 0: every work-group derives them on the device. Output is identical. */
#define RT_OPT_FRAME_CONSTS 4
/* RT_OPT_ORIGIN_LISTS (default 1): a secondary ray that starts on a sphere
 * of a scene of 33-256 spheres tests the candidates its direction selects in
 * that sphere's precomputed list instead of walking the sphere BVH
 * (depth >= 2); 0: every secondary ray walks the BVH. Output is identical. */
#define RT_OPT_ORIGIN_LISTS 7
/* RT_OPT_SCENE_SHAPES (default 1): a render whose scene has one of the
 * common shapes runs a kernel compiled for that shape, the way the
 * reference's shader is compiled for its own scene: at depth 0, shadow
 * queries that walk LDS direction masks (at most 64 spheres, 12-texel masks,
 * culling on; the mask width as a constant); at depth >= 2 without
 * Monte-Carlo, wide masks with their candidate lists and origin-sphere lists
 * (33-256 spheres, culling on); either with or without the room (exactly one
 * translate-only box holding every live light; its whole-frame depth-0
 * renders from inside it: RT_OPT_ROOM_FAST). 0: every render runs the
 * general kernel. Output is identical. */
#define RT_OPT_SCENE_SHAPES 8
/* RT_OPT_LAUNCH_SHAPES (default 1): a depth-0 render that runs a scene-shape
 * kernel and is a whole-frame float4 render — unsharded, all rows, the
 * RT_OUTPUT_RGBA32F surface, the host's frame constants (RT_OPT_FRAME_CONSTS),
 * at least 2 x 2 pixels, every view's camera within the short perspective
 * divisions' range, no accumulation — runs that kernel compiled for this
 * launch shape as well: none of the launch's own uniform tests (shard
 * mapping, surface format, division form) is made at run time. 0: every
 * render reads them at run time. Output is identical. */
#define RT_OPT_LAUNCH_SHAPES 9
/* RT_OPT_PERSISTENT0 (default 1): how a depth-0 rt_render_batch of more than
 * 8 views of one scene that takes the plain launch shape (RT_OPT_LAUNCH_SHAPES)
 * is distributed. 1: automatic — a grid of as many work-groups as are
 * resident at once, each staging the scene once, whose waves take chunks of
 * 8x8-pixel tiles from queues until the launch is done, when the launch has
 * at least 192 tiles per resident wave (49 frames of 1920x1080 on an
 * MI355X: below that the tiled launch measured faster); otherwise one
 * work-group per 16x16 tile. 0: always one work-group per tile. k >= 8: the resident grid whatever
 * the launch's size, of at most k work-groups (a development hook: small
 * frames then run the queue loop). Other values are refused. Output is
 * identical. */
#define RT_OPT_PERSISTENT0 10
/* RT_OPT_FIXED_LAYOUT (default 1): a scene with LDS shadow masks whose
 * lights, materials and boxes lie within its layout class's maxima (4 lights,
 * 8 materials, one box or up to 4) is staged in the class's fixed layout, and
 * its plain persistent launches (RT_OPT_PERSISTENT0) run the kernel that
 * takes the table offsets from the class instead of reading them per tile.
 * 0: every launch reads the offsets at run time; the scenes' blobs are the
 * same. Output is identical. */
#define RT_OPT_FIXED_LAYOUT 11
/* RT_OPT_ROOM_FAST (default 1): a depth-0 whole-frame float4 render
 * (RT_OPT_LAUNCH_SHAPES) of a room scene (RT_OPT_SCENE_SHAPES) whose room is
 * placed by a translation alone, with a normal matrix that leaves the face
 * axes as they are, and whose cameras all stand strictly inside it takes the
 * primary box hit
 * without the products by those matrices. A launch outside that proof, and
 * every launch with 0, runs the room kernels of the general launch shape.
 * Output is identical. */
#define RT_OPT_ROOM_FAST 12
/* RT_OPT_AA_QUEUED (default 1): how rt_render_aa*'s refine launch at depth 0
 * and 1 finds its work. 1: a resident grid whose waves take the live wave
 * tiles from the edge kernel's compact lists, as depths 2-9 always do. 0: one
 * work-group per 16 x 16 pixel tile, which leaves at once when none of its
 * pixels is flagged. Output is identical. */
#define RT_OPT_AA_QUEUED 13
/* (option 6, a tolerance tier that summed the recursion's colours forward
 * instead of mixing them on the way back up, measured even with the exact
 * walk and was removed: DESIGN.md §3.) */
/* (option 5, a level-by-level wavefront path for deep trees, was measured
 * 2x slower than the depth-first walk and removed: DESIGN.md §3.) */
int rt_context_set(rt_context *ctx, int option, int value);

/* Kernel-only timing of the last render call (ms, from HIP events around the
 * launch on its stream — around all of its launches when a deep batch is
 * split into several); needs RT_OPT_TIMING. */
int rt_last_kernel_ms(rt_context *ctx, float *ms);

/* RGBA8 unorm packing of a float frame as the shipped GL_RGBA8 surface stores
 * it (NaN -> 0, clamp to [0,1], v * 255 rounded to nearest even, as the
 * reference's GL converts; pinned by tests/golden/rgba8_llvmpipe.npz). Host
 * memory, n pixels. */
int rt_pack_rgba8(const float *rgba32f, size_t n_pixels, uint8_t *out_rgba8);

/* Headless image dump (replaces the display pass, draw_screen_*.glsl and
 * main.cpp:240-260). `rgba32f` is a frame in this ABI's layout (row 0 = GL's
 * bottom row). PPM: binary P6, 8-bit, RGBA8 unorm rounding (rt_pack_rgba8),
 * rows written top-down (the on-screen orientation). PFM: float RGB, rows
 * bottom-up as the PFM format stores them, little-endian. */
int rt_write_ppm(const char *path, const float *rgba32f, int width, int height);
int rt_write_pfm(const char *path, const float *rgba32f, int width, int height);

const char *rt_last_error(void);
const char *rt_version(void);

#ifdef __cplusplus
}
#endif
#endif
