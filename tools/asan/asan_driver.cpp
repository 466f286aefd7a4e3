// Host-only sanitizer driver (make -C openglraytracer_amd/csrc asan): runs
// the host C++ of the product — scene description parser, scene builder
// (masks, BVH, blob layout), per-frame constants, reference scene / camera,
// image dump — under AddressSanitizer + UndefinedBehaviorSanitizer, on the
// shipped scene descriptions, the benchmark scenes and a malformed-JSON
// corpus (every truncation of every scene file, seeded byte mutations, and
// hand-written edge cases). No GPU: nothing here launches a kernel.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../openglraytracer_amd/csrc/rt_internal.h"

namespace rtamd {
int build_scene(const rt_object *objs, int n_objs, const rt_material *mats, int n_mats, const rt_light *lights,
                int n_lights, std::vector<float4> &blob, DeviceScene &ds, bool with_origin_lists,
                double extent_floor = 0.0);
int build_origin_lists_for(const std::vector<float4> &host, const DeviceScene &ds, std::vector<uint8_t> &olist);
}  // namespace rtamd
// host-only development hooks (rt_scene.cpp)
extern "C" int rt_debug_anim_validate(const rt_object *base, const rt_object_anim *anim, const rt_anim_channel *radius,
                                      int n_objs, const rt_material *mats, int n_mats, const rt_light *lights,
                                      int n_lights, int max_frames, int boxes_only);
extern "C" long long rt_debug_anim_host_blob(const rt_object *base, const rt_object_anim *anim,
                                             const rt_anim_channel *radius, int n_objs, const rt_material *mats,
                                             int n_mats, const rt_light *lights, int n_lights, float time, void *out,
                                             long long cap, int32_t *meta);

namespace {

int g_parsed = 0, g_rejected = 0, g_built = 0;

void parse_and_build(const std::string &text, float t) {
    std::vector<rt_object> objs(RT_MAX_OBJECTS);
    std::vector<rt_material> mats(RT_MAX_MATERIALS);
    std::vector<rt_light> lights(RT_MAX_LIGHTS);
    rt_camera cam;
    int no = 0, nm = 0, nl = 0, hc = 0;
    if (rt_scene_desc_parse(text.c_str(), t, objs.data(), RT_MAX_OBJECTS, &no, mats.data(), RT_MAX_MATERIALS, &nm,
                            lights.data(), RT_MAX_LIGHTS, &nl, &cam, &hc) != RT_OK) {
        ++g_rejected;
        (void)rt_last_error();
        return;
    }
    ++g_parsed;
    std::vector<float4> blob;
    rtamd::DeviceScene ds;
    if (rtamd::build_scene(objs.data(), no, mats.data(), nm, lights.data(), nl, blob, ds, true) == RT_OK) {
        ++g_built;
        rt_view view;
        rt_make_view(hc ? &cam : nullptr, t, &view);
        rtamd::LaunchParams p{};
        p.n_views = 1;
        std::memcpy(p.view[0].unproj, view.unprojection, sizeof view.unprojection);
        std::memcpy(p.view[0].origin, view.origin, sizeof view.origin);
        p.view[0].cull = 1;
        p.width = 320;
        p.height = 180;
        p.layout = ds.layout;
        const float4 *blobs[1] = {blob.data()};
        rtamd::host_frame_setup(p, blobs);
    }
}

std::string slurp(const char *path) {
    std::ifstream f(path);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

}  // namespace

int main(int argc, char **argv) {
    // reference tables, benchmark scenes up to the object limit, cameras
    rt_material mats[RT_REFERENCE_MATERIALS];
    rt_light lights[RT_REFERENCE_LIGHTS];
    rt_reference_materials(mats);
    rt_reference_lights(lights);
    for (float t : {0.0f, 3.7f, -100.0f, 1e4f}) {
        rt_object ref[RT_REFERENCE_OBJECTS];
        rt_reference_objects(t, ref);
        std::vector<float4> blob;
        rtamd::DeviceScene ds;
        if (rtamd::build_scene(ref, RT_REFERENCE_OBJECTS, mats, RT_REFERENCE_MATERIALS, lights, RT_REFERENCE_LIGHTS,
                               blob, ds, true) != RT_OK)
            return 1;
        rt_view v;
        rt_make_view(nullptr, t, &v);
        // the same objects from the channel form (include/rt.h, rt_animate_objects)
        rt_object base[RT_REFERENCE_OBJECTS], anim_out[RT_REFERENCE_OBJECTS];
        rt_object_anim anim[RT_REFERENCE_OBJECTS];
        if (rt_reference_animation(base, anim) != RT_OK ||
            rt_animate_objects(base, anim, RT_REFERENCE_OBJECTS, t, anim_out) != RT_OK ||
            std::memcmp(anim_out, ref, sizeof ref) != 0)
            return 1;
    }
    for (int n : {0, 1, 16, 17, 33, 64, 65, 256, 257, RT_MAX_OBJECTS - 1}) {
        std::vector<rt_object> objs(n + 1);
        if (rt_bench_objects(n, 7, objs.data()) != RT_OK) return 1;
        std::vector<float4> blob;
        rtamd::DeviceScene ds;
        if (rtamd::build_scene(objs.data(), n + 1, mats, RT_REFERENCE_MATERIALS, lights, RT_REFERENCE_LIGHTS, blob,
                               ds, true) != RT_OK)
            return 1;
        ++g_built;
    }
    // the animate kernel's phases on the host (rt_anim_create2's host side, the
    // box and sphere phases over the kernel's table with the arithmetic of
    // rt_cull.h and rt_anim.h): config 2's scene with every sphere
    // moving and some breathing, and the shipped scene's boxes with its sphere
    // moving (box bits beside the sphere's); then the refusals
    for (int which = 0; which < 2; ++which) {
        std::vector<rt_object> base(17);
        std::vector<rt_object_anim> anim(17);
        int n = 17;
        if (which == 0) {
            if (rt_bench_objects(16, 3, base.data()) != RT_OK) return 1;
            std::memset(anim.data(), 0, anim.size() * sizeof(rt_object_anim));
        } else {
            n = RT_REFERENCE_OBJECTS;
            if (rt_reference_animation(base.data(), anim.data()) != RT_OK) return 1;
        }
        std::vector<rt_anim_channel> radius(n, rt_anim_channel{RT_ANIM_NONE, 0.0f, 0.0f, 0.0f});
        for (int i = 0; i < n; ++i) {
            const rt_object &o = base[i];
            if (o.box_mins[0] != 0.0f || o.box_maxs[0] != 0.0f) continue;  // (the boxes of these scenes)
            for (int k = 0; k < 3; ++k)
                anim[i].position[k] = rt_anim_channel{RT_ANIM_SIN_OFFSET, 0.5f + 0.1f * k, 0.7f + 0.05f * i, o.position[k]};
            if (i % 3 == 0) radius[i] = rt_anim_channel{RT_ANIM_SIN, 1.1f, 0.9f, 0.0f};  // (through 0, negative too)
        }
        if (rt_debug_anim_validate(base.data(), anim.data(), radius.data(), n, mats, RT_REFERENCE_MATERIALS, lights,
                                   RT_REFERENCE_LIGHTS, 4, 0) != RT_OK)
            return 1;
        for (float t : {0.0f, 1.25f, -40.0f}) {
            int32_t meta[24];
            const long long bytes = rt_debug_anim_host_blob(base.data(), anim.data(), radius.data(), n, mats,
                                                            RT_REFERENCE_MATERIALS, lights, RT_REFERENCE_LIGHTS, t,
                                                            nullptr, 0, meta);
            if (bytes <= 0) return 1;
            std::vector<unsigned char> out(static_cast<size_t>(bytes));
            if (rt_debug_anim_host_blob(base.data(), anim.data(), radius.data(), n, mats, RT_REFERENCE_MATERIALS,
                                        lights, RT_REFERENCE_LIGHTS, t, out.data(), bytes, meta) != bytes)
                return 1;
            ++g_built;
        }
        radius[n - 1].kind = 9;
        if (rt_debug_anim_validate(base.data(), anim.data(), radius.data(), n, mats, RT_REFERENCE_MATERIALS, lights,
                                   RT_REFERENCE_LIGHTS, 4, 0) != RT_ERR_INVALID)
            return 1;
    }
    {
        std::vector<rt_object> base(34);
        std::vector<rt_object_anim> anim(34);
        std::memset(anim.data(), 0, anim.size() * sizeof(rt_object_anim));
        if (rt_bench_objects(33, 3, base.data()) != RT_OK) return 1;
        anim[5].position[0] = rt_anim_channel{RT_ANIM_RATE, 0.0f, 0.01f, 0.0f};
        if (rt_debug_anim_validate(base.data(), anim.data(), nullptr, 34, mats, RT_REFERENCE_MATERIALS, lights,
                                   RT_REFERENCE_LIGHTS, 1, 0) != RT_ERR_UNSUPPORTED)
            return 1;
    }
    // image dump and RGBA8 packing (NaN / inf / negative values)
    std::vector<float> img(37 * 11 * 4);
    for (size_t i = 0; i < img.size(); ++i) img[i] = (i % 7 == 0) ? NAN : (i % 5 == 0 ? INFINITY : -0.5f + i * 0.01f);
    std::vector<uint8_t> rgba8(img.size());
    rt_pack_rgba8(img.data(), 37 * 11, rgba8.data());
    rt_write_ppm("/tmp/rt_asan.ppm", img.data(), 37, 11);
    rt_write_pfm("/tmp/rt_asan.pfm", img.data(), 37, 11);
    // scene descriptions: as shipped, every truncation, seeded mutations
    std::vector<std::string> files;
    for (int i = 1; i < argc; ++i) files.push_back(slurp(argv[i]));
    uint64_t st = 0x1234567;
    for (const std::string &text : files) {
        parse_and_build(text, 0.0f);
        parse_and_build(text, 2.5f);
        for (size_t cut = 0; cut < text.size(); ++cut) parse_and_build(text.substr(0, cut), 0.0f);
        for (int k = 0; k < 3000; ++k) {
            std::string m = text;
            for (int j = 0; j < 1 + k % 4; ++j) {
                st = st * 6364136223846793005ULL + 1442695040888963407ULL;
                const size_t at = (st >> 33) % (m.size() ? m.size() : 1);
                const char pool[] = "{}[]\":,-+.eE0123456789 \\nutlfa\x01\xff";
                const char c = pool[(st >> 20) % (sizeof pool - 1)];
                switch ((st >> 50) % 3) {
                    case 0: if (!m.empty()) m[at] = c; break;
                    case 1: m.insert(m.begin() + static_cast<long>(at), c); break;
                    default: if (!m.empty()) m.erase(at, 1 + (st >> 40) % 8); break;
                }
            }
            parse_and_build(m, 0.0f);
        }
    }
    const char *edge[] = {
        "", "{", "}", "[]", "null", "{\"objects\": [", "{\"objects\": [{}]}",
        "{\"objects\": [{\"sphere\": {\"position\": [1e400, 0, 0], \"radius\": 1, \"material\": 0}}]}",
        "{\"objects\": [{\"sphere\": {\"position\": [0, 0], \"radius\": 1}}]}",
        "{\"materials\": [], \"objects\": []}", "{\"lights\": [{\"position\": \"x\"}]}",
        "{\"camera\": {\"position\": [0,0,0], \"angles\": [0,0,0], \"v_fov\": -1e38}}",
        "{\"objects\": {\"bench\": {\"spheres\": 2147483647}}}", "{\"objects\": {\"bench\": {\"spheres\": -5}}}",
        "\"\\u12", "{\"a\": \"\\ud800\"}", "{\"objects\": [1, 2, 3]}",
    };
    for (const char *e : edge) parse_and_build(e, 0.0f);
    std::string deep(100000, '[');
    parse_and_build(deep, 0.0f);
    std::printf("asan driver: %d parsed, %d rejected, %d scenes built — clean\n", g_parsed, g_rejected, g_built);
    return 0;
}
