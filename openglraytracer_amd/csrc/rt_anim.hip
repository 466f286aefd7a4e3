// rt_anim.hip — the animate kernel: a scene's time-dependent parts rebuilt on
// the GPU, in stream order ahead of the render that reads them (include/rt.h,
// rt_anim; the reference moves its objects inside the shader from the uniform
// `time`, raytrace_compute.glsl:236-237, :261-321).
//
// One 256-thread work-group per frame rewrites, in that frame's slot blob,
// what build_scene (rt_scene.cpp) derives from the boxes' animated fields and
// nothing else:
//   1. records: one lane per box evaluates the channels (rt_anim.h) and the
//      reference GL's transform chain (rt_glmath.h, the text the host runs:
//      bit-identical) and stores the BoxRec's matrices, scaled extents,
//      w2l_w0 and translate_only; a lane of another wave the box's
//      light_inside and bounding sphere (float64);
//   2. the (box, light) separating planes (scenes of several boxes) and, for
//      the LDS direction masks' box bits, every (box, live light) cone;
//   3. the direction masks: one thread per texel ORs the boxes' bits into the
//      static spheres' template mask.
// Scenes with moving spheres (rt_anim_create2) run the kernel's second
// instance, animate_kernel<true>, which adds in the same phases, with the
// arithmetic of rt_anim.h and rt_cull.h (the text the host runs):
//   1. one lane per moving sphere: its SphereRec and SphereMeta::radius; one
//      lane per sphere slot, moving or not: its float64 box with build_bvh's
//      margin, in LDS;
//   2. one thread per BVH node: the node's six bounds, the union of the boxes
//      of its subtree's range of sphere slots (the topology, skip links, leaf words
//      and octant links stay the template's); per (moving sphere, light) the
//      ShadowCone where the layout has that table; per (moving sphere, live
//      light) the mask cone;
//   3. the moving spheres' bits in the direction masks, also in scenes
//      without box bits.
// Box-only scenes keep animate_kernel<false>, whose code carries none of that.
// Every record and every culling term (light_inside, balls, planes, cones,
// mask bits, BVH boxes) is rt_cull.h's function of the object, the text
// build_scene runs; the loops, the table and the stores are this file's. What
// passes through the float64 rotation need not equal the host's bit for bit
// (the device's double sin / cos may differ in the last place) and is as
// conservative: culling changes no pixel. Barriers only between the phases;
// every store is a plain vector store.
#include <hip/hip_runtime.h>

#include <cmath>

#include "rt_anim.h"

namespace rtamd {

namespace {

constexpr int kAnimThreads = 256;

// LDS: [flag, 16 B][n float4 balls][n x n_live MaskCone][n_spheres
// SphereBox, scenes with a moving sphere], n = the balls with mask bits
// the kernel recomputes (anim_mask_balls: the boxes' bounding spheres, then
// the moving spheres)
__host__ __device__ inline size_t lds_spheres_at() { return 16; }
__host__ __device__ inline size_t lds_cones_at(int n_balls) { return 16 + static_cast<size_t>(n_balls) * 16; }
__host__ __device__ inline size_t lds_boxes_at(int n_balls, int n_live) {
    return lds_cones_at(n_balls) + static_cast<size_t>(n_balls) * n_live * sizeof(MaskCone);
}

template <bool kSpheres>
__global__ __launch_bounds__(kAnimThreads) void animate_kernel(const AnimParams p) {
    extern __shared__ double lds_raw[];
    unsigned char *lds = reinterpret_cast<unsigned char *>(lds_raw);
    const AnimTable &T = *reinterpret_cast<const AnimTable *>(p.table);
    const int frame = blockIdx.x, tid = threadIdx.x;
    const float time = p.times[frame];
    unsigned char *blob = p.blobs + static_cast<size_t>((p.first_slot + frame) % p.n_slots) * p.slot_bytes;
    const int nb = T.n_boxes, nl = T.n_lights;
    const int n_mask_boxes = T.dmask_box ? nb : 0;
    const int n_ms = kSpheres ? T.n_msph : 0;
    const int n_balls = n_mask_boxes + (kSpheres && T.dmask_n > 0 ? n_ms : 0);
    int *bad = reinterpret_cast<int *>(lds);  // 1: an animated field the plane test looks at is not finite
    float4 *bsph = reinterpret_cast<float4 *>(lds + lds_spheres_at());
    MaskCone *cones = reinterpret_cast<MaskCone *>(lds + lds_cones_at(n_balls));
    SphereBox *sbox = reinterpret_cast<SphereBox *>(lds + lds_boxes_at(n_balls, T.n_live));
    const rt_object *base = reinterpret_cast<const rt_object *>(p.table + T.off_base);
    const rt_object_anim *anim = reinterpret_cast<const rt_object_anim *>(p.table + T.off_anim);
    const float4 *light = reinterpret_cast<const float4 *>(p.table + T.off_light);
    BoxRec *boxes = reinterpret_cast<BoxRec *>(blob + static_cast<size_t>(p.off_boxes) * 16);
    const AnimSphere *msph = reinterpret_cast<const AnimSphere *>(p.table + T.off_msph);
    SphereRec *sph = reinterpret_cast<SphereRec *>(blob + static_cast<size_t>(T.blob_spheres) * 16);
    SphereMeta *smeta = reinterpret_cast<SphereMeta *>(blob + static_cast<size_t>(T.blob_smeta) * 16);
    if (tid == 0) *bad = 0;
    __syncthreads();

    // ---- 1. records ------------------------------------------------------
    // The first half of the work-group runs the float32 chain, the second half
    // the float64 culling terms of the same boxes (other waves: side by side).
    // The halves store disjoint words of a BoxRec; obj_index, material and the
    // padding stay as build_scene laid them out.
    constexpr int kHalf = kAnimThreads / 2;
    if (tid < kHalf) {
        for (int b = tid; b < nb; b += kHalf) {
            const rt_object o = animate_object(base[b], anim[b], time);
            box_record(o, boxes[b]);
            bool finite = true;
            for (int r = 0; r < 3; ++r)
                finite = finite && isfinite(o.position[r]) && isfinite(o.box_mins[r]) && isfinite(o.box_maxs[r]);
            if (!finite) *bad = 1;
        }
        // the static spheres' boxes for the BVH refit, one lane per slot
        // (the moving spheres' lanes store theirs below)
        if (kSpheres && n_ms > 0)
            for (int s = tid; s < T.n_spheres; s += kHalf)
                if (!((T.moving_slots >> s) & 1u)) sbox[s] = anim_sphere_box(sph[s], smeta[s].radius, T.extent);
    } else {
        for (int b = tid - kHalf; b < nb; b += kHalf) {
            const rt_object o = animate_object(base[b], anim[b], time);
            double R[3][3];
            rotation64(o.angles, R);
            uint32_t inside = 0;
            for (int j = 0; j < nl && j < 32; ++j) {
                const float4 lj = light[j];
                const float lp[3] = {lj.x, lj.y, lj.z};
                if (light_inside_box(o, R, lp)) inside |= 1u << j;
            }
            boxes[b].light_inside = inside;
            if (b < n_mask_boxes) bsph[b] = box_ball(o, R);
        }
        if (kSpheres)
            for (int i = tid - kHalf; i < n_ms; i += kHalf) {
                const AnimSphere s = msph[i];
                SphereRec rec;
                float rad;
                anim_sphere_records(s, time, rec, rad);
                sph[s.slot] = rec;
                smeta[s.slot].radius = rad;
                sbox[s.slot] = anim_sphere_box(rec, rad, T.extent);
                if (n_balls > n_mask_boxes) bsph[n_mask_boxes + i] = make_float4(rec.cx, rec.cy, rec.cz, rad);
            }
    }
    __syncthreads();

    // ---- 2. planes and cones ---------------------------------------------
    if (p.off_bplane >= 0) {
        // per (box, light) the separating plane, in the float32 transform just stored
        float4 *bplane = reinterpret_cast<float4 *>(blob + static_cast<size_t>(p.off_bplane) * 16);
        const bool finite = T.finite && !*bad;
        for (int i = tid; i < nb * nl; i += kAnimThreads) {
            const float4 lj = light[i % nl];
            const float lp[3] = {lj.x, lj.y, lj.z};
            bplane[i] = finite ? box_light_plane(boxes[i / nl], lp, T.extent) : no_plane();
        }
    }
    for (int i = tid; i < n_balls * nl; i += kAnimThreads) {
        const int b = i / nl, j = i % nl;
        const float4 lj = light[j];
        const int li = __float_as_int(lj.w);
        if (li < 0) continue;  // a dead light has no mask
        const float4 s = bsph[b];
        const float ball[4] = {s.x, s.y, s.z, s.w}, lp[3] = {lj.x, lj.y, lj.z};
        int bit = T.n_spheres + b;
        if (kSpheres && b >= n_mask_boxes) bit = msph[b - n_mask_boxes].slot;
        cones[b * T.n_live + li] = mask_cone(ball, lp, bit);
    }
    if (kSpheres && n_ms > 0) {
        // the BVH's bounds, node by node, from the spheres' boxes
        const AnimNodeRange *range = reinterpret_cast<const AnimNodeRange *>(p.table + T.off_node);
        BvhNode *bvh = reinterpret_cast<BvhNode *>(blob + static_cast<size_t>(T.blob_bvh) * 16);
        for (int n = tid; n < T.n_bvh; n += kAnimThreads) {
            float lo[3], hi[3];
            anim_node_bounds(sbox, range[n], lo, hi);
            for (int a = 0; a < 3; ++a) {
                bvh[n].lo[a] = lo[a];
                bvh[n].hi[a] = hi[a];
            }
        }
        if (T.blob_cone >= 0) {
            // the ShadowCone table's entries of the moving spheres, every light's
            ShadowCone *scone = reinterpret_cast<ShadowCone *>(blob + static_cast<size_t>(T.blob_cone) * 16);
            for (int i = kAnimThreads - 1 - tid; i < n_ms * nl; i += kAnimThreads) {
                const int slot = msph[i / nl].slot, j = i % nl;
                const float4 lj = light[j];
                const float lp[3] = {lj.x, lj.y, lj.z};
                scone[j * T.n_spheres + slot] = shadow_cone(sph[slot], smeta[slot].radius, lp);
            }
        }
    }
    if (n_balls == 0) return;  // (uniform: every thread of the launch)
    __syncthreads();

    // ---- 3. direction masks: the texel test, texel by texel --------------
    const int texels = 6 * T.dmask_n * T.dmask_n;
    const double *cone_tab = reinterpret_cast<const double *>(p.table + T.off_cone);
    const unsigned char *tmpl = p.table + T.off_mask;
    unsigned char *dmask = blob + static_cast<size_t>(p.off_dmask) * 16;
    for (int i = tid; i < T.n_live * texels; i += kAnimThreads) {
        const int li = i / texels, t = i % texels;
        const double *w = cone_tab + 5 * static_cast<size_t>(t);
        uint64_t bits = 0;
        for (int b = 0; b < n_balls; ++b) {
            const MaskCone &c = cones[b * T.n_live + li];
            if (texel_hit(w, w[3], w[4], c)) bits |= uint64_t{1} << c.bit;
        }
        if (T.dmask_bytes == 2)
            reinterpret_cast<uint16_t *>(dmask)[i] =
                static_cast<uint16_t>(reinterpret_cast<const uint16_t *>(tmpl)[i] | bits);
        else if (T.dmask_bytes == 4)
            reinterpret_cast<uint32_t *>(dmask)[i] =
                static_cast<uint32_t>(reinterpret_cast<const uint32_t *>(tmpl)[i] | bits);
        else
            reinterpret_cast<uint64_t *>(dmask)[i] = reinterpret_cast<const uint64_t *>(tmpl)[i] | bits;
    }
}

}  // namespace

size_t animate_lds(const AnimTable &t) {
    const int n = anim_mask_balls(t);
    return lds_boxes_at(n, t.n_live) + (t.n_msph > 0 ? static_cast<size_t>(t.n_spheres) * sizeof(SphereBox) : 0);
}

hipError_t launch_animate(const AnimParams &p, bool spheres, int n_frames, size_t lds, hipStream_t stream) {
    if (spheres)
        hipLaunchKernelGGL(animate_kernel<true>, dim3(n_frames), dim3(kAnimThreads), lds, stream, p);
    else
        hipLaunchKernelGGL(animate_kernel<false>, dim3(n_frames), dim3(kAnimThreads), lds, stream, p);
    return hipGetLastError();
}

}  // namespace rtamd
