// rt_internal.h — shared declarations of the product library (host side).
//
// Layout of the device-resident scene (one hipMalloc'd blob per rt_scene, see
// rt_scene.cpp) and the per-launch parameter block consumed by the kernel in
// rt_kernel.hip. Everything is float32 / int32; offsets are in 16-byte units.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rt.h"

namespace rtamd {

// One sphere of the closest-hit loop: centre and radius*radius (the float
// product raytrace_compute.glsl:588 forms), 16 B.
struct SphereRec {
    float cx, cy, cz, rr;
};
// Identity of a sphere: its index in the reference object order (tie-break
// of get_closest_collision, :773) and its material.
struct SphereMeta {
    int32_t obj_index;
    int32_t material;
    float radius;  // |radius|, for the culling bounds (intersection uses rr)
    int32_t pad;
};

// One oriented box (:647-724) with its frame constants precomputed once per
// scene: world_to_local (:652), local_to_world (:650) and the normal matrix
// transpose(inverse(mat3(L))) (:718). Matrices are row-major 3x4 (the x/y/z
// rows of the GLSL mat4; the w row of an affine transform is (0,0,0,1)).
struct BoxRec {
    float w2l[12];
    float l2w[12];
    float nrm[9];
    float mins[3];
    float maxs[3];
    int32_t obj_index;
    int32_t material;
    uint32_t light_inside;  // bit j: light j strictly inside the box with margin (shadow shortcut)
    int32_t translate_only;  // w2l's 3x3 block is exactly the identity (world->local = + w2l[3,7,11])
    float w2l_w0[3];  // w2l[r][3] * 0.0f: the w column's term of (w2l * vec4(d, 0.0)) per row (+-0 or NaN)
    int32_t pad[2];
};  // 48 words = 192 B
static_assert(sizeof(BoxRec) == 192, "BoxRec layout");

// Material (:56-69) plus the per-material light products the shading loop
// would otherwise recompute: amb_sum = sum_j La_j * Ma (:801, same order),
// and for each light j: Ld_j * Md (:830), Ls_j * Ms (:832).
struct MatRec {
    float amb_sum[4];
    float emissive[4];
    float shininess, reflectivity, transparency, refraction_index;
    float eta_in, eta_out;  // 1.0 / refraction_index and 1.0 / that (:1013-1016), each correctly rounded
    float pad[2];
};  // 64 B
// The flags decide whether a light's direct term can change the Phong sums;
// the shadow ray is cast only then (lit and shadowed agree otherwise):
// d_nz / s_nz: some component of Ld*Md / Ls*Ms is nonzero; always: the
// material is not "tame" (a product is not finite, or the shininess is not a
// positive finite number), so the diffuse / specular factors may be NaN or
// infinite and every light's term is taken as changing the sums.
struct LightMatRec {
    float ld_md[4];
    float ls_ms[4];
    int32_t d_nz, s_nz, always, pad;
};  // 48 B
// Shadow-ray culling cone of sphere s seen from light j (host, float64):
// v = unit direction light -> centre; far = d - rp where d = |centre - light|
// and rp = |radius| + 0.021 + 1e-3 d (the 0.01 start offset plus margins);
// sin / cos of the half-angle asin(rp / d); near = 1 when d <= rp (the light
// is inside the inflated sphere: always a candidate).
struct ShadowCone {
    float v[3];
    float far;
    float sph, cph, near, pad;
};  // 32 B
constexpr size_t kConeLdsBudget = 24 * 1024;
// Shadow-ray direction masks (scenes of at most 64 spheres): for every light
// that casts shadow rays (not `dead`), a cube map of 6 x n x n texels around
// the light; texel bit s is set when some direction of the texel lies within
// sphere s's inflated cone from the light (the ShadowCone geometry, float64,
// plus the texel's own angular radius and a margin). A shadow ray whose
// direction from the light falls in the texel can only be blocked by the
// spheres of its mask. Face f = 2 * axis + (component < 0); within the face
// the two other axes in increasing order give (column, row). Kept while the
// work-group's LDS stays within kMaskLdsBudget (full occupancy); masks are
// 16, 32 or 64 bits wide (scenes of at most 16, 32, 64 spheres).
constexpr int kMaskMaxSpheres = 64;
constexpr size_t kMaskLdsBudget = 19 * 1024;
// Larger scenes (up to kGMaskMaxSpheres) use the same masks as 64-bit words
// per texel, kGMaskTexels per face edge, in the device blob after the part
// the work-groups stage (read through L2: 256 spheres, 768 KB per live light at 64 texels).
constexpr int kGMaskMaxSpheres = 256;
#ifndef RT_GMASK_TEXELS
#define RT_GMASK_TEXELS 64  // tuning knob (tools/ablate.sh flags); 8/16/24/32/48/64: config 4 28.2/25.9/25.2/25.0/24.9/24.8 ms
                            // (r01); after the ordered BVH 32/48/64: 18.29/17.91/17.73 ms, config 3 1.002/1.005/0.996 ms
#endif
constexpr int kGMaskTexels = RT_GMASK_TEXELS;
// The same wide masks as short candidate lists, one 16-B record per (live
// light, texel): byte 0 = the number of candidate spheres (0..15), bytes
// 1..15 = their slots (< 256), the sphere of the largest angular size from
// the light first (rt_scene.cpp); kGListOverflow in byte 0: more than
// 15 candidates, use the texel's mask words. A query then walks its own list:
// a wave loops max-over-lanes-of-count times, once per candidate, instead of
// once per set bit per mask word (the sum over the words of the per-word
// maxima), from one 16-B load instead of one 8-B load per word.
constexpr int kGListMax = 15;
constexpr uint32_t kGListOverflow = 255u;
static_assert(kGMaskMaxSpheres <= 256, "candidate lists hold sphere slots in bytes");
// Secondary rays that start on a sphere (round 5; tools/model/
// origin_list_model.py: 66-73 % of config 4's secondary rays, 58 % of
// config 3's) look up the spheres they can hit instead of walking the BVH:
// per sphere s, a cube map of kOListTexels x kOListTexels texels per face
// (direction_texel's layout) whose texel lists every sphere j that a ray
// from the ball B(c_s, r_s + 0.001) — every reflection or refraction origin
// on s (:1010-1023) — with its direction in the texel can hit: the cone of
// the texel from c_s meets the ball B(c_j, r_j + r_s + 0.001) (the shadow
// masks' test, float64, with margins), s itself first (a ray inside s
// leaves through it). The candidates follow in increasing order of a lower
// bound of their hit distance, |c_j - c_s| - r_j - r_s - margins, so a lane
// whose closest hit so far (the box's, tested first) lies below the next
// bound can stop. One 32-B record per (sphere, texel):
//   byte 0      the number of candidates (255: 255 or more);
//   bytes 1..25 the first kOListSlots candidates' sphere slots;
//   bytes 26..31 three uint16 bounds in 1/256 units (rounded down, 65535 at
//               most): of candidate 8, of candidate 16, and of candidate
//               kOListSlots (the first one not in the record; 65535 when
//               there is none). A lane checks the first two before testing
//               candidates 8 and 16; one that has tested the whole record
//               and still lies above the third walks the BVH instead.
// Built for scenes of kOListMinSpheres..kGMaskMaxSpheres spheres, read by the
// recursive kernels (depth >= 2) through L2, never staged.
#ifndef RT_OLIST_TEXELS
#define RT_OLIST_TEXELS 16
#endif
constexpr int kOListTexels = RT_OLIST_TEXELS;
constexpr int kOListSlots = 25;
constexpr int kOListRecordBytes = 32;
#ifndef RT_OLIST_FROM
#define RT_OLIST_FROM 33  // (the wide masks' threshold: smaller scenes keep the BVH walk, their blob unchanged)
#endif
constexpr int kOListMinSpheres = RT_OLIST_FROM;
constexpr float kOListBoundUnit = 1.0f / 256.0f;
// Sphere BVH node (depth-first order; the left child is the next node):
// lo = (min xyz, skip) and hi = (max xyz, leaf) where skip is the node after
// this subtree (-1: end) and leaf = (count << 24) | first sphere slot (0 for
// an inner node). Bounds are the spheres' boxes inflated by a margin far
// above float error, so the approximate box test never drops a sphere the
// exact test could hit.
struct BvhNode {
    float lo[3];
    int32_t skip;
    float hi[3];
    int32_t leaf;
};
static_assert(sizeof(BvhNode) == 32, "BvhNode layout");
// Ordered traversal of the closest-hit walk: per node, 8 link words, one per
// ray-direction octant (bit a set: d[a] < 0), each (next node on a hit) |
// (next node on a miss) << 16, 0xFFFF = end. The octant's depth-first order
// enters every inner node's children nearer-first along its split axis, so
// near hits shrink the search interval before the far subtree is tested.
constexpr int kBvhOctants = 8;

struct LightRec {
    float pos[3];
    float dead;  // 1: zero diffuse and specular for every material (no direct term, no shadow ray)
};

// Per-launch parameters (kernarg, read through the scalar cache).
// Per-frame camera constants of one view of a launch.
struct FrameView {
    float unproj[16];  // column-major inverse(proj*view) (:383)
    float proj[16];    // column-major proj*view = inverse(unproj) (float64 on the host), for culling
    float origin[3];   // ray start = camera position (:391)
    int32_t cull;      // 1: exactness-preserving culling enabled (consistent pinhole view)
    // The camera ray's terms that depend on the view and the frame size alone,
    // from the host (fill_view) for the plain launches (camera_ray<kLaunchPlain>):
    // every wave tile computed them again on the vector pipe, uniform as they
    // are (no scalar float unit). The same floats as the device's:
    //  * unproj_half[k] = unproj[8 + k] * 0.5f, one IEEE multiplication on
    //    either side (the kernel is built without contraction);
    //  * rcp_hw, rcp_hh = 1.0f / float(W / 2), 1.0f / float(H / 2), IEEE on the
    //    host; the device's rcp_refined(b).r is the correctly rounded 1 / b for
    //    every significand (tools/probes/arith_probe.hip, exhaustive), so the
    //    same float. (Its Rcp::b, float(W / 2), is exact and stays on the device.)
    // A frame 1 pixel wide or high has inf here; no plain launch is one.
    float unproj_half[4];
    float rcp_hw, rcp_hh;
    const void *blob;  // this view's scene blob (rt_render_batch_scenes); nullptr: LaunchParams::scene
};
static_assert(sizeof(FrameView) == 176 && offsetof(FrameView, unproj_half) % 16 == 0, "FrameView: whole 16-B units");
// (-DRT_HOST_VIEW_TERMS=0: a timing build whose plain launches compute the
// terms on the device, tools/ablate.sh flags)
#ifndef RT_HOST_VIEW_TERMS
#define RT_HOST_VIEW_TERMS 1
#endif
constexpr bool kHostViewTerms = RT_HOST_VIEW_TERMS != 0;
constexpr int kMaxViews = 8;  // frames per launch (blockIdx.z) with the views in the kernel arguments
// Larger batches (up to RT_MAX_BATCH views, depth 0-1): the views and their
// frame constants go to a per-context device buffer (one of kBatchSlots,
// reused behind an event), read by render_kernel<D, false, true>.
constexpr int kBatchSlots = 4;
// per-frame constant records carried in the kernel arguments: all views'
// (8 views of 16 spheres + 1 box = 264), at most kMaxViewConsts per view
// (one record per thread of a work-group)
constexpr int kMaxFrameConsts = 272;
constexpr int kMaxViewConsts = 256;
// Largest LDS a work-group may request on gfx950 (160 KiB).
constexpr size_t kMaxLds = 160 * 1024;

// The layout of a scene blob: its sections' offsets in 16-B units, the mask
// parameters and the counts. The single definition: build_scene fills it, the
// host's frame constants and the kernels read it (LaunchParams::layout), and
// two scenes may share a launch when theirs are equal (rt_render_batch_scenes).
// All int32 and nothing else, so equality is a comparison of the bytes.
struct SceneLayout {
    int32_t off_spheres, off_smeta, off_boxes, off_mats, off_lights, off_lightmat;
    int32_t off_bvh, n_bvh;  // sphere BVH nodes (2 x float4 each), offset / count
    int32_t off_blink;       // n_bvh x kBvhOctants uint32 traversal links
    int32_t off_cone;        // n_lights x n_spheres ShadowCone; -1: none
                             // (kept only while the LDS total stays within kConeLdsBudget)
    int32_t off_dmask, dmask_n;  // shadow direction masks (live lights x 6 x n x n); -1: none
    int32_t dmask_bytes;         // bytes per mask: 2, 4 or 8 (at most 16, 32, 64 mask bits; 4 without masks)
    int32_t off_gmask, gmask_words;  // wide masks in the blob past blob_units (not staged); -1: none
    int32_t off_glist;               // their candidate lists (kGListMax); -1: none
    int32_t blob_units;      // the part every work-group stages into LDS
    // secondary rays' origin-sphere candidate lists (kOListSlots); -1: none,
    // or not built yet (ensure_origin_lists)
    int32_t off_olist;
    // 1: the LDS direction masks carry a bit per box (bit n_spheres + b)
    int32_t dmask_box;
    // per (box, light) a plane that separates the box from the light's end
    // of every shadow segment (rt_scene.cpp), n_boxes x n_lights float4; -1: none
    int32_t off_bplane;
    int32_t n_spheres, n_boxes, n_mats, n_lights;
};

struct LaunchParams {
    FrameView view[kMaxViews];
    int32_t n_views;
    int32_t width, height;
    int32_t row_begin, n_rows;          // contiguous band [row_begin, row_begin+n_rows)
    int32_t block_rows, n_shards, shard;  // interleaved shard mapping when n_shards > 0
    const void *scene;  // device blob
    float4 *out;        // n_views x n_rows x width float4
    // Monte-Carlo accumulation (render_kernel<D, true>): samples
    // [sample0, sample0 + spp) per pixel, jittered inside the pixel when
    // jitter != 0, summed in sample order and added to out.
    int32_t spp, sample0, jitter;
    uint32_t seed;
    // The layout of `scene`, and of every view's own blob. It sits behind
    // `seed` for the persistent kernel, which reads the arguments again per
    // tile: the compiler merges neighbouring scalar loads into wider ones from
    // wherever a run of loaded words begins. Here the first four offsets lie on
    // a 16-B boundary, and no word a depth-0 tile reads comes right before the
    // offsets or right after the counts. (With the counts first and the layout
    // ahead of the pointers the kernel read n_lights and three offsets in one
    // unaligned 16-B load and took one load more per tile.)
    SceneLayout layout;
    // Queued work distribution (rt_kernel.hip, render_kernel): the counters of
    // this launch (kSchedInts zeroed ints, left zeroed by the kernel).
    // nullptr: one work-group per tile.
    int32_t *sched;
    int32_t out_format;  // RT_OUTPUT_*: float4, GL_RGBA8 unorm bytes (uchar4) or packed float3 per pixel
    // Each view's per-frame constants ([sphere camera terms][sphere pixel
    // footprints][box camera terms], the LDS image the kernel's frame_setup
    // derives), computed on the host when all views' fit here
    // (host_frame_setup): n_frame_consts records per view, view k's at
    // k * n_frame_consts; 0: every work-group derives them.
    int32_t n_frame_consts;
    // 1: every view's camera-ray perspective divisions take the short form,
    // exact for every pixel (rt_scene.cpp camera_short_divisions)
    int32_t cam_short;
    // Rows [slice_begin, slice_begin + slice_rows) of the launch's local rows
    // (the whole launch when slice_rows = 0).
    int32_t slice_begin, slice_rows;
    // 1: the launch's room proof holds (LaunchHost::room_fast, kRoomFast): the
    // general depth-0 colour kernels take the room fast path. (In the padding
    // ahead of the pointers: the block's size and every other offset stand.)
    int32_t room_fast;
    // > kMaxViews views (render_kernel<D, false, true>): n_views FrameViews
    // and n_views x n_frame_consts records in device memory; nullptr: the
    // arrays above
    const FrameView *views_dev;
    const float4 *consts_dev;
    // (last: kernarg_probe reads the block's end)
    float4 frame_consts[kMaxFrameConsts];
};
static_assert(sizeof(LaunchParams) == 5968, "kernel argument block: the hidden arguments' offsets");
static_assert(offsetof(LaunchParams, layout) % 16 == 0, "the layout's offsets: aligned scalar loads (see above)");
static_assert(offsetof(LaunchParams, frame_consts) + sizeof(LaunchParams::frame_consts) == sizeof(LaunchParams),
              "kernarg_probe reads the last record: nothing the kernels read lies behind it");
// ROCm passes kernel arguments above 4 KiB (an 8 KB argument block checked on
// MI355X); this block stays under 6 KiB.
static_assert(sizeof(LaunchParams) <= 6144, "kernel argument block");
// What the host decides a launch's kernel and grid from, beside the argument
// block (no kernel reads it): base_params fills it from the context and the
// scene, scene_shape / launch_shape / persistent_groups read it.
struct LaunchHost {
    // 1 when every view of the launch culls (and RT_OPT_SCENE_SHAPES is on),
    // so the kernels may take the scene's shape (scene_shape)
    int32_t shape_cull;
    int32_t scene_room;  // every scene of the launch is a room (DeviceScene::room)
    // The room proof of the launch (kRoomFast): every scene's record passes
    // room_record_identity (DeviceScene::room_fast), every view's host-made
    // box record room_view_inside, and RT_OPT_ROOM_FAST is on. launch_shape
    // gives a room scene the plain launch only with it.
    int32_t room_fast;
    // RT_OPT_LAUNCH_SHAPES: the depth-0 shaped kernels may take the launch's
    // shape (launch_shape)
    int32_t shape_launch;
    // RT_OPT_PERSISTENT0 (0 off, 1 automatic, k >= 8: forced, at most k
    // work-groups; persistent_groups), 0 too when a view of the batch carries
    // a scene blob of its own (rt_render_batch_scenes)
    int32_t persistent0;
    // RT_OPT_FIXED_LAYOUT: a launch of a scene in its class's fixed layout may
    // take the kernels that read the class's offsets (kShapeFixed)
    int32_t fixed_layout;
    int32_t n_cu;  // the compute units a resident grid is sized for; 0: tiled launches only
};
// Scene shapes (render_kernel<D, ..., kShape>): the scene's features that
// decide the path a ray takes, as compile-time constants, so the kernel
// carries none of their run-time tests. Depth 0: the LDS direction masks'
// bytes (2, 4, 8; culling on, so every shadow query walks them). Depth >= 2:
// kShapeWide (culling on; wide masks with their candidate lists and the
// origin-sphere lists present). Either | kShapeRoom (exactly one box, a room:
// translate-only, every live light inside it).
// 0: everything read at run time. Chosen per launch on the host
// (scene_shape), like the reference's shader, compiled for its own scene.
constexpr int kShapeMaskBytes = 15;
constexpr int kShapeMaskTexels = 12;  // the LDS masks' texels per face edge in a depth-0 shape (rt_scene.cpp picks 12 where it fits)
constexpr int kShapeRoom = 16;
constexpr int kShapeWide = 32;
// kShapeFixed (with an LDS-mask shape; the persistent kernels): the staged
// blob has its layout class's fixed layout (fixed_layout below), so the
// kernel takes its table addresses from the class instead of reading
// LaunchParams::layout per wave tile. Never with RT_OPT_FIXED_LAYOUT 0.
constexpr int kShapeFixed = 64;
// The room fast path (rt_kernel.hip closest_impl / resolve_impl<true, true>):
// the kernels of the room shape on a plain launch (kShapeRoom, kLaunchPlain;
// depth 0, no accumulation) take the primary box hit without the products by
// the box's identity matrices. launch_shape gives a room scene the plain
// launch only with the host's proof (LaunchHost::room_fast), so no kernel is
// added; a launch without it runs the room kernels of the general launch.
// The general depth-0 colour kernels (RT_OPT_SCENE_SHAPES 0, or a scene
// without LDS masks) read the proof's answer from LaunchParams::room_fast.
// Which launch took the path: kernel_takes_room_fast below.
// (-DRT_ROOM_FAST=0: a timing build whose plain room kernels keep the general
// code and whose launches do not ask for the proof, tools/ablate.sh flags)
#ifndef RT_ROOM_FAST
#define RT_ROOM_FAST 1
#endif
constexpr bool kRoomFast = RT_ROOM_FAST != 0;
// Round 18: the host also proves the operands of the path's inverse square
// roots inside the short forms' ranges (norm_proof_scene, camera_norm_range
// below), so the kernels that take the path call the short forms without their
// per-wave range votes; the proofs join the launch's room proof
// (LaunchHost::room_fast). (-DRT_NORM_PROOFS=0: a timing build in which no such
// proof is asked for and the votes stay, tools/ablate.sh flags)
#ifndef RT_NORM_PROOFS
#define RT_NORM_PROOFS 1
#endif
constexpr bool kNormProofs = kRoomFast && RT_NORM_PROOFS != 0;
// Timing builds that price an instruction of the persistent depth-0 kernel
// (-DRT_PAD_SALU=n, -DRT_PAD_VALU=n, tools/ablate.sh flags; rt_kernel.hip
// persistent_pad): n more scalar or vector adds per tile. DESIGN.md §3, round 18.
#ifndef RT_PAD_SALU
#define RT_PAD_SALU 0
#endif
#ifndef RT_PAD_VALU
#define RT_PAD_VALU 0
#endif
constexpr int kPadSalu = RT_PAD_SALU, kPadValu = RT_PAD_VALU;
// The proof's scene half, on the room's record. The 3x3 blocks of w2l and l2w
// are the identity (1.0f, and zeros of either sign: with the view half no
// zero's sign in them reaches a result, DESIGN.md §3 "Arithmetic"), their
// translation columns are finite (w2l_w0 then holds zeros), and the normal
// matrix takes each of the six signed face axes the kernel forms (resolve_impl:
// the axis, or the axis times -1.0f) to the vector the fast path writes: the
// sign at the face's place and +0 elsewhere, bit for bit. The signs of the
// normal matrix' zeros decide that last part (the reference's own transform
// chain leaves -0 in places), so it is evaluated here as the kernel does.
inline bool room_record_identity(const BoxRec &b) {
    const auto bits = [](float f) {
        uint32_t u;
        std::memcpy(&u, &f, sizeof u);
        return u;
    };
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            const float want = r == c ? 1.0f : 0.0f;
            if (b.w2l[r * 4 + c] != want || b.l2w[r * 4 + c] != want) return false;
        }
        if (!std::isfinite(b.w2l[r * 4 + 3]) || !std::isfinite(b.l2w[r * 4 + 3]) || b.w2l_w0[r] != 0.0f) return false;
    }
    for (int face = 0; face < 3; ++face)
        for (const float sign : {1.0f, -1.0f}) {
            float n[3] = {face == 0 ? 1.0f : 0.0f, face == 1 ? 1.0f : 0.0f, face == 2 ? 1.0f : 0.0f};
            if (sign < 0.0f)
                for (float &x : n) x = x * -1.0f;
            for (int r = 0; r < 3; ++r) {
                const float *N = b.nrm + 3 * r;
                const float v = N[0] * n[0] + N[1] * n[1] + N[2] * n[2];
                if (bits(v) != bits(r == face ? sign : 0.0f)) return false;
            }
        }
    return true;
}
// The proof's view half, on the view's own record of the box (the kernel's
// box_cam: the box-local camera origin, w = 1 when strictly inside): inside,
// finite, and no component a negative zero.
inline bool room_view_inside(const float4 &box_cam) {
    const float v[3] = {box_cam.x, box_cam.y, box_cam.z};
    for (const float f : v)
        if (!std::isfinite(f) || (f == 0.0f && std::signbit(f))) return false;
    return box_cam.w == 1.0f;
}
// The scene half of the norm proofs (kNormProofs; the view half is
// rt_scene.cpp camera_norm_range). With it, at every primary hit of a room
// launch the operands of normalize(sdir) (phong_impl) and of the sphere
// normal (resolve_impl) lie inside inv_sqrt's [2^-96, 2^100] by twenty binades
// or more, so the short forms need no vote. DESIGN.md §3 "Arithmetic" derives
// the terms; in short, with B the largest |coordinate| of the room, the
// spheres (centre +- radius) and the live lights, all in float64:
//  * e2 = 2^-12 B^2 bounds | |p - C|^2 - r^2 | for the float32 hit point p of
//    a sphere (C, r) from a camera inside the room: the discriminant's
//    rounding, at most 2^-13.9 B^2, reaches the squared distance at most
//    1.25-fold, grazing hits included;
//  * gap = 2^-12 B: a wall's hit point is within 2^-20 B of its plane;
//  * so: B <= 2^20; every |r| in [2^-20, 2^20] with r^2 >= 2 e2 (the normal's
//    operand stays above e2 >= 2^-52); every live light at least gap from each
//    wall plane, and its distance from C outside
//    [sqrt(r^2 - e2) - gap, sqrt(r^2 + e2) + gap] for each sphere.
// Then |sdir| >= gap - 2^-20 B >= 2^-33 and |sdir| <= 4 B <= 2^22.
struct NormProof {
    int32_t ok = 0;
    double bound = 0.0, e2 = 0.0, gap = 0.0;
};
inline NormProof norm_proof_scene(const BoxRec &room, const SphereRec *sph, const SphereMeta *meta, int n_spheres,
                                  const LightRec *lights, int n_lights) {
    NormProof r;
    double lo[3], hi[3], B = 0.0;
    for (int k = 0; k < 3; ++k) {
        lo[k] = double(room.mins[k]) + double(room.l2w[4 * k + 3]);
        hi[k] = double(room.maxs[k]) + double(room.l2w[4 * k + 3]);
        B = std::fmax(B, std::fmax(std::fabs(lo[k]), std::fabs(hi[k])));
    }
    for (int s = 0; s < n_spheres; ++s) {
        const double c[3] = {sph[s].cx, sph[s].cy, sph[s].cz}, rad = std::fabs(double(meta[s].radius));
        for (const double x : c) B = std::fmax(B, std::fabs(x) + rad);
    }
    for (int j = 0; j < n_lights; ++j)
        if (lights[j].dead == 0.0f)
            for (const float x : lights[j].pos) B = std::fmax(B, std::fabs(double(x)));
    if (!(B > 0.0 && B <= 0x1p20)) return r;  // (a NaN fails)
    r.bound = B;
    r.e2 = 0x1p-12 * B * B;
    r.gap = 0x1p-12 * B;
    for (int s = 0; s < n_spheres; ++s) {
        const double rad = std::fabs(double(meta[s].radius));
        // (the kernel's rr is the float product of the radius with itself)
        if (!(rad >= 0x1p-20 && rad <= 0x1p20 && rad * rad >= 2.0 * r.e2 && double(sph[s].rr) >= 2.0 * r.e2)) return r;
    }
    for (int j = 0; j < n_lights; ++j) {
        if (lights[j].dead != 0.0f) continue;
        const double L[3] = {lights[j].pos[0], lights[j].pos[1], lights[j].pos[2]};
        for (int k = 0; k < 3; ++k)
            if (!(std::fabs(L[k] - lo[k]) >= r.gap && std::fabs(L[k] - hi[k]) >= r.gap)) return r;
        for (int s = 0; s < n_spheres; ++s) {
            const double dx = L[0] - sph[s].cx, dy = L[1] - sph[s].cy, dz = L[2] - sph[s].cz;
            const double d = std::sqrt(dx * dx + dy * dy + dz * dz), rr = double(meta[s].radius) * double(meta[s].radius);
            const bool outside = d >= std::sqrt(rr + r.e2) + r.gap, inside = d <= std::sqrt(rr - r.e2) - r.gap;
            if (!outside && !inside) return r;
        }
    }
    r.ok = 1;
    return r;
}
// Layout classes of the LDS-mask scenes. A class is one box or several; inside
// it the tables a depth-0 shaped kernel reads sit at offsets that are a
// function of the class and the sphere count alone: first the tables whose
// sizes the class fixes — the boxes (1 or kFixedMaxBoxes records), the
// materials, the lights and the light x material records, each padded to its
// maximum — then the spheres, their meta records and the masks (whose size
// follows the live lights), then what the shaped kernels do not address by
// the class (the planes, whose place tests/anim_spheres_common.py fixes right
// before the BVH, the BVH and its links). The sphere tables are not padded to
// the mask bits: config 2's scene with 40 spheres has 144 B to spare under
// kMaskLdsBudget, so any padding of them (768 B to 64 spheres) would cost it
// its 12-texel masks. Their count is read per tile anyway, so the meta
// records and the masks sit at a class constant plus n_spheres and 2 n_spheres
// units. For the same 144 B the maxima of the materials and lights are the
// reference's own tables' sizes, 7 and 3: one material more is 208 B
// (a MatRec and three LightMatRec), one light more 352 B. Rows of light x
// material records keep n_lights records each. build_scene pads a scene that
// is inside the maxima and whose mask texels the padding does not change
// (kMaskLdsBudget); every other scene keeps the compact layout. The class
// follows from the object kinds and the counts alone, so the frames of an
// animated scene share it.
constexpr int kFixedMaxLights = 3, kFixedMaxMats = 7, kFixedMaxBoxes = 4;
struct FixedLayout {
    int32_t off_boxes, off_mats, off_lights, off_lightmat, off_spheres;
    // the meta records and the masks of a scene of n spheres
    __host__ __device__ constexpr int32_t off_smeta(int n) const { return off_spheres + n; }
    __host__ __device__ constexpr int32_t off_dmask(int n) const { return off_spheres + 2 * n; }
};
static_assert(sizeof(SphereRec) == 16 && sizeof(SphereMeta) == 16, "a unit per sphere and table");
__host__ __device__ constexpr FixedLayout fixed_layout(bool one_box) {
    FixedLayout f{};
    f.off_boxes = 0;
    f.off_mats = f.off_boxes + (one_box ? 1 : kFixedMaxBoxes) * static_cast<int>(sizeof(BoxRec) / 16);
    f.off_lights = f.off_mats + kFixedMaxMats * static_cast<int>(sizeof(MatRec) / 16);
    f.off_lightmat = f.off_lights + kFixedMaxLights * static_cast<int>(sizeof(LightRec) / 16);
    f.off_spheres = f.off_lightmat + kFixedMaxMats * kFixedMaxLights * static_cast<int>(sizeof(LightMatRec) / 16);
    return f;
}
// The counts of a class: one box or 2..kFixedMaxBoxes, lights and materials
// within their maxima, spheres (and the boxes' bits) within the masks' 64 bits.
inline bool fixed_counts(int n_spheres, int n_boxes, int n_mats, int n_lights) {
    return n_spheres >= 1 && n_boxes >= 1 && n_boxes <= kFixedMaxBoxes && n_lights >= 1 &&
           n_lights <= kFixedMaxLights && n_mats >= 1 && n_mats <= kFixedMaxMats &&
           n_spheres + (n_boxes >= 2 ? n_boxes : 0) <= kMaskMaxSpheres;
}
// L is its class's fixed layout (the class of its own boxes).
inline bool layout_is_fixed(const SceneLayout &L) {
    if (L.off_dmask < 0 || !fixed_counts(L.n_spheres, L.n_boxes, L.n_mats, L.n_lights)) return false;
    const FixedLayout f = fixed_layout(L.n_boxes == 1);
    return L.off_boxes == f.off_boxes && L.off_mats == f.off_mats && L.off_lights == f.off_lights &&
           L.off_lightmat == f.off_lightmat && L.off_spheres == f.off_spheres &&
           L.off_smeta == f.off_smeta(L.n_spheres) && L.off_dmask == f.off_dmask(L.n_spheres);
}
int scene_shape(const SceneLayout &L, const LaunchHost &h, int max_depth);
// Launch shapes (render_kernel<D, ..., kShape, kLaunch>, the depth-0 shaped
// kernels without accumulation): the launch's own uniform answers as
// compile-time constants, a bit per shape; 0: everything read at run time.
// kLaunchPlain, the whole-frame float4 render (rt_render's draw, an unsharded
// rt_render_batch): whole unsharded rows (n_shards <= 0, row_begin = 0,
// n_rows = height, one slice), the RGBA32F surface, cam_short = 1, the host's
// frame constants present, width and height >= 2. Chosen per launch on the
// host (launch_shape) from the parameters alone; RT_OPT_LAUNCH_SHAPES 0
// (LaunchHost::shape_launch) forces 0.
constexpr int kLaunchPlain = 1;
// kLaunchPersistent (only with kLaunchPlain, on the device-view kernels): the
// resident-grid distribution of a depth-0 batch of one scene (rt_kernel.hip,
// "Work distribution"). Needs the kernel's resident work-groups, so
// launch_shape reports it only for a launch whose `resident` is known.
constexpr int kLaunchPersistent = 2;
int launch_shape(const LaunchParams &p, const LaunchHost &h, int max_depth, int resident = 0);
// Wave tiles a persistent wave takes per dequeue in the bulk of the launch
// (kChunk0 consecutive items, view-major; a power of two): 256 frames of 1080p
// need about 1,300 tiles per microsecond and one counter serves about 88
// dequeues per microsecond, so the 32 heads at 16 tiles each run at a
// thirtieth of their ceiling. A dequeue is a round trip the wave waits for,
// a division of the item number and, at 1080p (2,025 chunks of 16 per view),
// mostly a refill of the wave's view records too; with the tail below, config
// 2 at 1080p per frame, chunks of 8 / 16 / 32: 256 views 24.6 / 24.3 / 24.4 us,
// 128 views 25.1 / 24.9 / 25.2, 64 views 25.6 / 25.6 / 26.0
// (profiles/r09c_ab_chunk_size.log; chunks of 4: +2.8 % at 256).
#ifndef RT_CHUNK0
#define RT_CHUNK0 16
#endif
constexpr int kChunk0 = RT_CHUNK0;
static_assert(kChunk0 >= 2 && kChunk0 <= 32 && (kChunk0 & (kChunk0 - 1)) == 0, "bulk chunk: a power of two, 2..32");
// The persistent launch's schedule: chunk id c -> items [t, t_end) of `total`
// on a grid of `waves` waves (the one function the kernel and the host-only
// rt_debug_persistent_chunk call). Chunk sizes fall towards the end of the
// launch: the bulk in chunks of kChunk0, then a region of chunks of
// kChunk0 / 2, ... , of 2 and last of single tiles. The region of size s ends
// where s * waves items are left, so it holds about a chunk per wave (the
// singles two per wave), and a wave that takes the last chunk of size s has
// s items per wave of smaller chunks behind it for the others: no wave runs
// more than about a tile past the rest (a wave tile takes 4 to 22 us of a
// wave's time with 8 waves on its SIMD, 10 us on average: the SIMD issues
// oldest wave first, so its youngest waves are its slowest all launch long).
// That holds only because a wave takes its next chunk when it needs it
// (render_persistent0). A launch smaller than its tail has the later regions
// only. Ids past the last chunk
// give an empty range. total < 2^30 (persistent_groups), so nothing here
// leaves int: the region sizes come from total / s, never from s * waves.
struct ChunkRange {
    int t, t_end;
};
__host__ __device__ inline ChunkRange persistent_chunk(int c, int total, int waves) {
    int start = 0;
#pragma unroll
    for (int s = kChunk0; s >= 2; s >>= 1) {
        const int left = (total - start) / s - waves;  // chunks of s before s * waves items are left
        const int n = left > 0 ? left : 0;
        if (c < n) return {start + c * s, start + c * s + s};
        c -= n;
        start += n * s;
    }
    return c < total - start ? ChunkRange{start + c, start + c + 1} : ChunkRange{total, total};
}
// A chunk's items are consecutive wave tiles, view-major and row by row, so
// they fall into runs: maximal stretches within one tile row of one view,
// tiles (wx .. wx + n - 1, wy) of view z. What is the same for every tile of a
// run (the view and its records, the row's terms, the store's row) the kernel
// derives once per run; inside it only wx advances. (-DRT_TILE_RUNS=0: a
// timing build that derives everything per tile, as before the runs.) The
// one pair of functions the kernel and the host-only rt_debug_persistent_runs
// call: the run that item t begins (the one division of a chunk), and the
// run behind a run that ended at its row's last tile or at the chunk's end.
// wtx x wty: the frame's wave tiles; `left`: the chunk's items from the run's
// first on (> 0).
#ifndef RT_TILE_RUNS
#define RT_TILE_RUNS 1
#endif
constexpr bool kTileRuns = RT_TILE_RUNS != 0;
struct TileRun {
    int z, wy, wx, n;
};
__host__ __device__ inline TileRun persistent_first_run(int t, int left, int wtx, int wty) {
    const int view_tiles = wtx * wty;
    const int z = t / view_tiles, r = t - z * view_tiles;
    const int wy = r / wtx, wx = r - wy * wtx;
    return {z, wy, wx, left < wtx - wx ? left : wtx - wx};
}
// (the run before ended at its row's last tile: `left` > 0 items are still the chunk's)
__host__ __device__ inline TileRun persistent_next_run(const TileRun &r, int left, int wtx, int wty) {
    const bool last_row = r.wy + 1 == wty;
    return {last_row ? r.z + 1 : r.z, last_row ? 0 : r.wy + 1, 0, left < wtx ? left : wtx};
}
// Automatic persistence (RT_OPT_PERSISTENT0 1) from this many wave tiles per
// resident wave. Measured on config 2 at 1080p, tiled -> persistent per
// launch: 9 views (36 tiles per wave) 270 -> 300 us, 16: 454 -> 467, 24:
// 665 -> 668, 32: 877 -> 864, 48 (190 per wave): 1296 -> 1257, 64: 1714 ->
// 1645, 128: 3379 -> 3190, 256: 6.67 -> 6.26 ms
// (profiles/r09f_persistent_threshold.log). Through 9 and 256 views the
// tiled launch costs 36 us + 25.9 us per view, the persistent one 83 us +
// 24.1 us per view: it pays from about 26 views now (from 40 with the first
// schedule); the threshold has not been moved yet.
constexpr int kPersistentMinTilesPerWave = 192;
// Work-groups of the persistent grid for a plain depth-0 launch on a kernel
// with `resident` resident work-groups on the device, 0: the tiled launch.
int persistent_groups(const LaunchParams &p, const LaunchHost &h, int resident);
// Lean views (the wide-shape recursive kernels): a view's records in LDS are
// its footprints and box terms only, not the spheres' camera terms (the
// primary rays compute them as secondary rays do: the same arithmetic, so the
// same values) — 16 B less per sphere per view.
constexpr bool kLeanViews(int shape) { return (shape & kShapeWide) != 0; }
// 16-B records of one view's per-frame constants in LDS: the spheres' camera
// terms (not with lean views) and footprints, the boxes' camera terms.
inline int view_units(const SceneLayout &L, bool lean) { return (lean ? 1 : 2) * L.n_spheres + L.n_boxes; }
constexpr int kQueues = 32;                            // wave-tile queues of a queued launch
constexpr int kQueueStride = 64;                       // ints: each counter on a 256-B line of its own
constexpr int kSchedInts = 2 * kQueues * kQueueStride; // heads + done counters of one launch
constexpr int kSchedSlots = 64;                        // launches that may be in flight at once
// The persistent launch's waves and queues. Work-groups go to the chip's
// eight XCDs in turn, so with queue g % kQueues every queue was served by the
// waves of one XCD (and one SIMD index) alone and an eighth of the launch's
// chunks was tied to each XCD, whatever its speed: the queues ran dry up to
// 190 us apart at 256 views of 1080p (profiles/r09a_persistent_trace.log).
// Round r = g / kQueues of the grid's waves is therefore dealt to the queues
// rotated by kQueueRotate0 * r (odd, so over kQueues rounds a wave slot of
// the chip serves every queue): every round still maps onto the queues one to
// one, so a grid of kQueues waves or more leaves no queue without a wave, and
// the wave's first chunk is its round's chunk of its queue.
#ifndef RT_QUEUE_ROTATE0
#define RT_QUEUE_ROTATE0 5
#endif
constexpr int kQueueRotate0 = RT_QUEUE_ROTATE0;
static_assert((kQueues & (kQueues - 1)) == 0, "the queue arithmetic masks with kQueues - 1");
__host__ __device__ inline int persistent_queue(int g) { return (g + kQueueRotate0 * (g / kQueues)) & (kQueues - 1); }
// Waves of queue q on a grid of `waves` waves: one per whole round, and one
// more where the last, partial round reaches the queue.
__host__ __device__ inline int persistent_queue_waves(int q, int waves) {
    const int rounds = waves / kQueues, rest = waves & (kQueues - 1);
    return rounds + (((q - kQueueRotate0 * rounds) & (kQueues - 1)) < rest ? 1 : 0);
}
// The chunk wave g starts with: the g / kQueues-th of its queue. The queue's
// head then hands out the chunks from persistent_queue_waves on.
__host__ __device__ inline int persistent_first_chunk(int g) { return (g & ~(kQueues - 1)) + persistent_queue(g); }

struct DeviceScene {
    void *blob = nullptr;
    SceneLayout layout{};  // (off_olist -1 until the lists are built: ensure_origin_lists)
    int32_t olist_eligible = 0;  // kOListMinSpheres..256 spheres: depth >= 2 renders get the lists
    // 1: the one box is a room: translate-only, every live light strictly
    // inside it (the shadow queries' box shortcut always applies; kShapeRoom)
    int32_t room = 0;
    int32_t room_fast = 0;  // a room whose record passes room_record_identity (kRoomFast)
    // room_fast, and the scene passes norm_proof_scene (kNormProofs). A scene
    // whose spheres the device moves (rt_anim) never claims it: the proof reads
    // the spheres where the host put them.
    NormProof norm;
};

// rt_scene.cpp: every view's per-frame constants on the host, bit-identical
// to the kernel's frame_setup for the camera terms (float32, same operation
// order) and conservative pixel footprints; view k's 2 * n_spheres + n_boxes
// records (from its scene's host blob, blobs[k]) go to p.frame_consts at
// k * p.n_frame_consts, p.n_frame_consts = records per view, or 0 when they
// do not all fit.
void host_frame_setup(LaunchParams &p, const float4 *const *blobs);
// One view's records for a device-side batch (render_batch_impl, > kMaxViews
// views): writes 2 * n_spheres + n_boxes records of view V (p: the launch's
// scene parameters) to out; the record count, or 0 if it exceeds
// kMaxViewConsts (then every work-group derives them).
int host_view_consts(const LaunchParams &p, const FrameView &V, const float4 *blob, float4 *out);
// A view's kernel-side constants (unprojection, proj for culling, origin,
// cull flag); false if its perspective divisions may not take the short form.
bool fill_view(const rt_context *ctx, const rt_view &view, int width, int height, FrameView &out);
// rt_scene.cpp: the view half of the norm proofs (kNormProofs), see there
bool camera_norm_range(const float M[16], int width, int height);

// rt_camera.cpp: the reference orbit camera as llvmpipe evaluates it
float gl_sin(float a);  // gallivm's polynomial sin / cos (run-time GLSL sin / cos)
float gl_cos(float a);
void reference_orbit(float time, float *speed, float pos[3], float *yaw);
void reference_view_gl(float time, float unproj[16], float view[16]);
// a box object's local_to_world, world_to_local and normal matrix as
// llvmpipe evaluates intersect_box_object (column-major)
void reference_box_transforms(const float pos[3], const float ang[3], float l2w[16], float w2l[16], float nrm[9]);

// rt_kernel.hip. The render kernels stand in one table, a row per
// instantiation of render_kernel<depth, accum, dev, shape, launch> (shape:
// kShape* bits, launch: kLaunch* bits) with the kernel's address.
struct KernelKey {  // (five int32_t and no padding: the debug hooks copy it out as such)
    int32_t depth, accum, dev, shape, launch;
};
struct KernelRow {
    KernelKey key;
    void (*kernel)(LaunchParams);
    const void *fn() const { return reinterpret_cast<const void *>(kernel); }  // as the HIP runtime takes it
};
const KernelRow *find_kernel(const KernelKey &k);  // null: no such instantiation
// The kernel a launch takes: `tiled` (or queued), and for a depth-0 batch
// where `candidate` is set `persistent` instead when persistent_groups, at
// that kernel's resident work-groups, gives a grid. False: a launch no kernel
// serves (device-side views above depth 1 or with accumulation).
struct KernelChoice {
    KernelKey tiled, persistent;
    bool candidate;
};
bool select_kernel(const LaunchParams &p, const LaunchHost &h, int max_depth, KernelChoice &c);
// The launch of row k with parameters p takes the room fast path.
inline bool kernel_takes_room_fast(const KernelKey &k, const LaunchParams &p) {
    if (!kRoomFast || k.depth != 0 || k.accum) return false;
    if (k.shape == 0) return p.room_fast != 0;
    return (k.shape & kShapeRoom) != 0 && (k.launch & kLaunchPlain) != 0;
}
// Launches the row select_kernel names (`ran`: its key). Clears p.sched when
// the launch does not use the queued distribution (so the caller knows
// whether the counter slot is in use).
hipError_t launch_render(LaunchParams &p, const LaunchHost &h, int max_depth, hipStream_t stream, KernelKey &ran);
// LDS of a one-view work-group: the blob's staged part and the view's records.
size_t lds_bytes(const SceneLayout &L, bool lean = false);
// Views of one scene a queued launch at this depth holds (deep frames: every
// view's per-frame constants beside the scene in LDS at the one-view
// launch's occupancy), 1..kMaxViews; 1 below the queued depths.
int queued_views(const SceneLayout &L, int max_depth);
// Self-test of the kernel argument block on the context's stream (rt_create).
int check_kernarg_block(hipStream_t stream);
// The primary-hit kernel's second argument (rt_render_hits*, rt_pick): the
// planes it writes, one 16-B record per pixel of the launch's rows each
// (nullptr: the plane is not wanted), and the RT_HITS_* flags. The launch
// itself travels in LaunchParams as for a render (one view, rows
// [row_begin, row_begin + n_rows), no shards); LaunchParams::out is not read.
struct HitTargets {
    int4 *hits;       // rt_hit: object, t, shadow mask, material
    float4 *normals;  // (n, 0); a miss (0, 0, 0, 0)
    float4 *points;   // (p, 0); a miss (0, 0, 0, 0)
    int32_t flags;
    int32_t pad;
};
static_assert(sizeof(HitTargets) == 32 && sizeof(LaunchParams) + sizeof(HitTargets) <= 6144, "kernel argument block");
// Launches hits_kernel (not a row of the render table: select_kernel and
// find_kernel do not know it), tiled, on `stream`.
hipError_t launch_hits(LaunchParams &p, const HitTargets &o, hipStream_t stream);
// Adaptive anti-aliasing (rt_render_aa*; rt_aa.h has the criterion). A call's
// scratch, per context: the wave tiles' 64-bit masks (aa_mask_slot's order),
// the compact lists of the live tiles (wy * tiles_x + wx, in the order the
// edge kernel's waves arrive) and their counters, zeroed on the call's stream.
// One list with one counter took 25 ns per live tile (two atomics on one
// line: 75 us of edge kernel for config 2's 2,974 live tiles at 1080p, 725 us
// for config 3's 30,756 at 2160p), so there are kAaQueues lists, each with a
// counter on a 256-B line of its own, as the render kernels' queues have
// theirs. Work-group tile g (row-major) appends to list g % kAaQueues: the
// lists are spatially interleaved and hold at most aa_queue_cap tiles each.
constexpr int kAaQueues = 32;
static_assert((kAaQueues & (kAaQueues - 1)) == 0 && kAaQueues <= 32, "masked with kAaQueues - 1; polled by one half-wave");
struct AaQueue {
    // one atomic per live tile adds (its flagged pixels << 32) | 1: the low
    // word is the list's length (and the tile's place in it), the high word
    // the flagged pixels of the list's tiles (a frame has at most 2^32 pixels)
    unsigned long long count;
    int32_t head;  // the refine launch's item counter
    int32_t pad[61];
};
static_assert(sizeof(AaQueue) == 256, "a counter per 256-B line");
// Tiles a list holds at most: four per work-group tile of its share.
inline int aa_queue_cap(int width, int height) {
    const long long groups = static_cast<long long>((width + 15) / 16) * ((height + 15) / 16);
    return static_cast<int>((groups / kAaQueues + 1) * 4);
}
// The second kernel argument of the edge and refine kernels, as HitTargets is
// the hits kernel's; LaunchParams is unchanged.
struct AaTargets {
    unsigned long long *masks;
    int32_t *list;  // kAaQueues x queue_cap
    AaQueue *queues;
    uint8_t *refined;  // one byte per pixel, 1 = flagged; nullptr: not wanted
    float threshold;
    int32_t queue_cap;
};
static_assert(sizeof(AaTargets) == 40 && sizeof(LaunchParams) + sizeof(AaTargets) <= 6144, "kernel argument block");
// The edge kernel over the frame at p.out (p.width x p.height float4), one
// wave per wave tile: masks, list, counters and the refined plane.
hipError_t launch_aa_edge(const LaunchParams &p, const AaTargets &a, hipStream_t stream);
// The refine launch (not a row of the render table): the general Monte-Carlo
// body over the flagged pixels, p.spp jittered samples from sample 0 with
// p.seed, their mean stored over the base pixel at p.out. Tiled (depths 0-1
// with queued01 false): a work-group per 16 x 16 tile that leaves when its
// four masks are zero. Queued (depths 2-9 always): a resident grid (h.n_cu)
// that takes the live tiles from the lists.
hipError_t launch_aa_refine(LaunchParams &p, const AaTargets &a, const LaunchHost &h, int max_depth, bool queued01,
                            hipStream_t stream);
// Ray queries (rt_trace_rays, rt_view_rays): the second kernel argument of the
// ray kernels, as HitTargets is the hits kernel's. `rays`: two 16-B records per
// ray (origin, direction; the w components are never read). The colour kernel
// writes `colors`, the hits kernel the three other planes (nullptr: not
// wanted), one 16-B record per ray each. Of LaunchParams the ray kernels read
// `scene` and `layout` only: no view, no frame constants, no output pointer.
struct RayTargets {
    const float4 *rays;
    float4 *colors;   // (r, g, b, 0)
    int4 *hits;       // rt_hit
    float4 *normals;  // (n, 0); a miss (0, 0, 0, 0)
    float4 *points;   // (p, 0); a miss (0, 0, 0, 0)
    int64_t n_rays;   // 1..RT_MAX_RAYS
    int32_t flags;    // RT_HITS_*
    int32_t cull;     // RT_OPT_CULLING
};
static_assert(sizeof(RayTargets) == 56 && sizeof(LaunchParams) + sizeof(RayTargets) <= 6144, "kernel argument block");
// A caller's ray may walk the approximate pre-tests of the closest-hit search
// (the sphere BVH's node test) only while its origin lies within this many
// units of the world's origin on every axis: rt_kernel.hip node_hit derives
// the bound (the node test stays conservative to about 4,000 units; a quarter
// of that is taken). And only while its direction is a unit vector up to
// rounding, | |d|^2 - 1 | <= 2^-19: its reflection and refraction children
// keep its length, and the origin-sphere lists' stored distance bounds are
// compared with their ray parameters (rt_scene.cpp origin_lists_range allows
// 1e-5 of the length; 2^-20 here, and about 1e-6 more over nine bounces). A
// wave that holds a ray outside either runs with culling off, for the ray's
// whole tree and its shading: every box and every sphere tested exactly,
// which the closest hit and the shadow queries do not notice.
// (-DRT_RAY_NEAR_ORIGIN=1e30f: a probe build whose far origins walk the BVH, to
// see tests/test_gpu_rays.py's far set fail; never the product build)
#ifndef RT_RAY_NEAR_ORIGIN
#define RT_RAY_NEAR_ORIGIN 1024.0f
#endif
constexpr float kRayNearOrigin = RT_RAY_NEAR_ORIGIN;
constexpr float kRayUnitDir = 0x1p-19f;
// rays_kernel<max_depth> over o.n_rays rays (colours), 256 rays per work-group.
hipError_t launch_rays(LaunchParams &p, const RayTargets &o, int max_depth, hipStream_t stream);
// ray_hits_kernel over o.n_rays rays (hits, normals, points).
hipError_t launch_ray_hits(LaunchParams &p, const RayTargets &o, hipStream_t stream);
// Occlusion queries (rt_occluded): the second kernel argument of
// occluded_kernel. `rays` as RayTargets has them, read as segments origin +
// t * dir, 0 < t < 1. `bytes`: one byte per ray (1 occluded, 0 not); `words`:
// bit i % 64 of word i / 64, (n_rays + 63) / 64 words; either may be nullptr.
struct OccludedTargets {
    const float4 *rays;
    uint8_t *bytes;
    uint64_t *words;
    int64_t n_rays;  // 1..RT_MAX_RAYS
    int32_t cull;    // RT_OPT_CULLING
    int32_t pad;
};
static_assert(sizeof(OccludedTargets) == 40 && sizeof(LaunchParams) + sizeof(OccludedTargets) <= 6144,
              "kernel argument block");
// occluded_kernel over o.n_rays segments, 256 per work-group (rt_kernel.hip
// segment_walk_slack derives when a segment walks the sphere BVH).
hipError_t launch_occluded(LaunchParams &p, const OccludedTargets &o, hipStream_t stream);
// view_rays_kernel: the camera rays of p.view[0] for rows [p.row_begin,
// p.row_begin + p.n_rows) of a p.width x p.height frame, in pixel order.
hipError_t launch_view_rays(const LaunchParams &p, float4 *rays, hipStream_t stream);

// rt_api.cpp
void set_error(const std::string &msg);
int hip_fail(const char *what, hipError_t e);  // sets the message, returns RT_ERR_HIP
// The event a render call records after its launch on a caller stream, shared
// by every scene the call reads (a batch of 256 animated frames with a scene
// each records one event, not 256: round 6, the shipped workload's host gap
// of 1.2 ms per launch) and destroyed with its last user (a pending event is
// released once complete).
struct UseEvent {
    hipEvent_t ev = nullptr;
    UseEvent() = default;
    UseEvent(const UseEvent &) = delete;
    UseEvent &operator=(const UseEvent &) = delete;
    ~UseEvent() {
        if (ev) (void)hipEventDestroy(ev);
    }
};
int check_render_args(const rt_context *ctx, const rt_scene *scene, int width, int height, int max_depth);
// launch parameters of n_views views of `scene` on `ctx` (output and rows left
// to the caller) and, in h, the host's side of the launch decisions
LaunchParams base_params(const rt_context *ctx, const rt_scene *scene, const rt_view *views, int n_views,
                         int width, int height, LaunchHost &h);
// launch on `stream` with the context's queue slot; span: between kernel-time events of its own
int launch(rt_context *ctx, LaunchParams &p, const LaunchHost &h, int max_depth, hipStream_t stream, bool span = true);
// Before a render at max_depth: a scene that reads origin-sphere lists at
// this depth (max_depth >= 2, RT_OPT_ORIGIN_LISTS on, 33-256 spheres) gets
// them built and appended to its device blob the first time (the region past
// the blob the earlier renders read; a larger blob is reallocated and the old
// one freed behind its renders). One host build + synchronous upload per
// scene contents; RT_OK at once when nothing is needed.
int ensure_origin_lists(rt_context *ctx, const rt_scene *scene, int max_depth);
// a render on `stream` reads `scene`'s blob: remember it (an event on that
// stream) so that rt_scene_destroy / rt_scene_update wait for it
// `shared`: the render call's event (created and recorded after its launch
// by the first scene noted, then reused for the call's other scenes); nullptr:
// an event of this call alone
int note_scene_use(const rt_scene *scene, hipStream_t stream, std::shared_ptr<UseEvent> *shared = nullptr);
// a render call's launch of views of one scene: launch, then note_scene_use
int launch_scene(rt_context *ctx, const rt_scene *scene, LaunchParams &p, const LaunchHost &h, int max_depth,
                 hipStream_t stream);
// bytes per pixel of a surface format (RT_OUTPUT_*)
inline size_t surface_bytes(int fmt) { return fmt == RT_OUTPUT_RGBA8 ? 4 : (fmt == RT_OUTPUT_RGB32F ? 12 : 16); }
// A grow-only device buffer of `units` units of `unit` bytes: reserve frees and
// allocates anew when it has to grow (hipFree waits for the device, so an
// earlier call's use of the old block is over) and never shrinks (rt_api.cpp).
struct DeviceBuffer {
    size_t unit = sizeof(float4);
    void *ptr = nullptr;
    size_t units = 0;
    float4 *records() const { return static_cast<float4 *>(ptr); }
    int reserve(size_t n, const char *what);  // what: hip_fail's label
    void release();
};

}  // namespace rtamd

struct rt_context {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    rtamd::DeviceBuffer staging;       // host-destination renders: a float4 per pixel (serves every format)
    rtamd::DeviceBuffer hits_staging;  // the same for rt_render_hits*: three planes of a record per pixel
    // the same for rt_trace_rays / rt_view_rays with host buffers: the rays (two
    // 16-B units each) and the wanted planes behind them
    rtamd::DeviceBuffer rays_staging;
    int aa_queued = 1;  // RT_OPT_AA_QUEUED
    // adaptive anti-aliasing (rt_render_aa*): one device allocation, in bytes,
    // [queue counters][masks][lists][refined plane of a host-destination call],
    // sized for aa_slots mask slots (whole work-group tiles) and aa_px pixels; the
    // event follows the last call's use of it (and of `staging`), and the next
    // call's stream waits for it on the device
    rtamd::DeviceBuffer aa_scratch{1};
    size_t aa_slots = 0, aa_px = 0;
    hipEvent_t aa_done = nullptr;
    bool aa_used = false;
    bool timed = false;
    int culling = 1;  // RT_OPT_CULLING
    int timing = 1;   // RT_OPT_TIMING
    int output = RT_OUTPUT_RGBA32F;  // RT_OPT_OUTPUT
    int host_consts = 1;  // RT_OPT_FRAME_CONSTS
    int origin_lists = 1;  // RT_OPT_ORIGIN_LISTS
    int scene_shapes = 1;  // RT_OPT_SCENE_SHAPES
    int launch_shapes = 1;  // RT_OPT_LAUNCH_SHAPES
    int persistent0 = 1;  // RT_OPT_PERSISTENT0
    int fixed_layout = 1;  // RT_OPT_FIXED_LAYOUT
    int room_fast = 1;  // RT_OPT_ROOM_FAST
    bool last_room_fast = false;  // the last launch took the room fast path (rt_debug_last_room_fast)
    // device-side view batches (> kMaxViews views): per slot a device buffer,
    // its pinned host staging and an event after the last launch that read it
    void *batch_dev[rtamd::kBatchSlots] = {};
    void *batch_host[rtamd::kBatchSlots] = {};
    hipEvent_t batch_done[rtamd::kBatchSlots] = {};
    bool batch_used[rtamd::kBatchSlots] = {};
    unsigned batch_next = 0;
    int n_cu = 0;               // compute units of the device
    int32_t *sched = nullptr;   // kSchedSlots x kSchedInts queue counters (zeroed)
    unsigned sched_next = 0;    // next slot: launches in flight on several streams use distinct slots
    // per slot: an event recorded after the slot's last queued launch; a
    // launch that reuses the slot waits for it on its own stream, so more
    // than kSchedSlots queued launches in flight never share counters
    hipEvent_t sched_done[rtamd::kSchedSlots] = {};
    bool sched_used[rtamd::kSchedSlots] = {};
    bool last_queued = false;   // the last launch used its slot (rt_debug_last_queued)
    int last_shape = 0;         // the last launch's scene shape (rt_debug_last_scene_shape)
    rtamd::KernelKey last_kernel{};  // the row the last launch ran (rt_debug_last_kernel)
    std::vector<struct rt_scene *> scenes;  // live scenes (detached by rt_destroy)
};

struct rt_scene {
    int device = 0;
    rtamd::DeviceScene dev;
    std::vector<float4> host;    // host copy of the blob (per-frame constants on the host)
    int32_t capacity_units = 0;  // allocated blob size (16-B units)
    rt_context *ctx = nullptr;   // owning context (nullptr once it is destroyed)
    // Renders that read the blob on streams other than the owning context's:
    // per stream, an event recorded after its latest such render. The blob
    // is freed or overwritten only behind all of them (stream order covers
    // the context's own stream). More than kMaxUseStreams streams: `overflow`,
    // and the release synchronises the device instead.
    static constexpr int kMaxUseStreams = 8;
    using Event = rtamd::UseEvent;
    struct Use {
        hipStream_t stream;
        std::shared_ptr<Event> done;
    };
    mutable std::vector<Use> uses;
    mutable bool overflow = false;
    mutable bool warned = false;  // the overflow's one-time stderr notice was printed
};
