// rt_cli — headless frame driver: the counterpart of the reference's
// main()/draw() loop (OpenGLRaytracer/main.cpp:47-93, :210-261) without a
// window. Renders the shipped scene (or a benchmark scene) at `time`, K frames
// apart by `dt` (the orbiting camera and animated boxes, :334-364, :261-321),
// and writes each frame as PPM (what the RGBA8 surface shows) and/or PFM.
//
//   rt_cli [--width 1280] [--height 720] [--depth 0] [--time 0] [--frames 1]
//          [--dt 0.016] [--scene shipped|spheres:N[:seed]|FILE.json] [--ppm out_%04d.ppm]
//          [--pfm out_%04d.pfm] [--hits PREFIX] [--aa SPP[:THRESHOLD]] [--device 0]
//          [--gpus N [--transport rccl|copy] [--block-rows 8]]
//
// --aa SPP[:THRESHOLD] renders every frame through rt_render_aa: pixels on a
// colour edge (a 4-neighbour differing by more than THRESHOLD, 0.1 when
// omitted, in some channel) become the mean of SPP jittered samples (seed 0).
// One GPU only.
// --hits PREFIX also writes every frame's primary-hit buffers (rt_render_hits)
// as three PFMs: PREFIX.hit.pfm (object index, t, shadow mask, as floats),
// PREFIX.normal.pfm and PREFIX.point.pfm (PREFIX may hold a %d for the frame
// number). One GPU only.
// --gpus N renders every frame on devices device..device+N-1 with
// rt_render_multi (row blocks per GPU, RCCL gather to the first GPU).
#include <chrono>
#include <fstream>
#include <sstream>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt.h"

namespace {

int fail(const char *what) {
    std::fprintf(stderr, "rt_cli: %s: %s\n", what, rt_last_error());
    return 1;
}

std::string frame_name(const std::string &pattern, int k) {
    if (pattern.find('%') == std::string::npos) return pattern;
    char buf[4096];
    std::snprintf(buf, sizeof buf, pattern.c_str(), k);
    return buf;
}

}  // namespace

int main(int argc, char **argv) {
    int width = 1280, height = 720, depth = 0, frames = 1, device = 0;  // main.cpp:17-19
    int gpus = 1, block_rows = 8, transport = RT_MULTI_RCCL;
    float time0 = 0.0f, dt = 1.0f / 60.0f;
    std::string scene = "shipped", ppm, pfm, hits;
    int aa_spp = 0;  // --aa: samples per flagged pixel; 0: one ray per pixel
    float aa_threshold = 0.1f;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char * {
            if (i + 1 >= argc) { std::fprintf(stderr, "rt_cli: %s needs a value\n", a.c_str()); std::exit(2); }
            return argv[++i];
        };
        if (a == "--width") width = std::atoi(next());
        else if (a == "--height") height = std::atoi(next());
        else if (a == "--depth") depth = std::atoi(next());
        else if (a == "--time") time0 = std::strtof(next(), nullptr);
        else if (a == "--frames") frames = std::atoi(next());
        else if (a == "--dt") dt = std::strtof(next(), nullptr);
        else if (a == "--scene") scene = next();
        else if (a == "--ppm") ppm = next();
        else if (a == "--pfm") pfm = next();
        else if (a == "--hits") hits = next();
        else if (a == "--aa") {  // SPP[:THRESHOLD]
            const char *v = next();
            char *end = nullptr;
            aa_spp = static_cast<int>(std::strtol(v, &end, 10));
            if (end && *end == ':') aa_threshold = std::strtof(end + 1, &end);
            if (aa_spp < 1 || !end || *end != '\0' || end == v) {
                std::fprintf(stderr, "rt_cli: --aa takes SPP[:THRESHOLD] with SPP >= 1\n");
                return 2;
            }
        }
        else if (a == "--device") device = std::atoi(next());
        else if (a == "--gpus") gpus = std::atoi(next());
        else if (a == "--block-rows") block_rows = std::atoi(next());
        else if (a == "--transport") transport = std::strcmp(next(), "copy") == 0 ? RT_MULTI_COPY : RT_MULTI_RCCL;
        else {
            std::fprintf(stderr, "usage: rt_cli [--width W] [--height H] [--depth D] [--time T] [--frames K] "
                                 "[--dt S] [--scene shipped|spheres:N[:seed]|FILE.json] [--ppm PAT] [--pfm PAT] "
                                 "[--hits PREFIX] [--aa SPP[:THRESHOLD]] [--device I] [--gpus N] [--transport rccl|copy] [--block-rows B]\n");
            return 2;
        }
    }
    if (gpus < 1) { std::fprintf(stderr, "rt_cli: --gpus must be >= 1\n"); return 2; }
    if (!hits.empty() && gpus > 1) { std::fprintf(stderr, "rt_cli: --hits renders on one GPU (not with --gpus above 1)\n"); return 2; }
    if (aa_spp > 0 && gpus > 1) { std::fprintf(stderr, "rt_cli: --aa renders on one GPU (not with --gpus above 1)\n"); return 2; }
    std::vector<rt_context *> ctxs(gpus, nullptr);
    for (int g = 0; g < gpus; ++g)
        if (rt_create(device + g, &ctxs[g]) != RT_OK) return fail("rt_create");
    rt_context *ctx = ctxs[0];
    rt_multi *group = nullptr;
    if (gpus > 1 && rt_multi_create(gpus, ctxs.data(), transport, &group) != RT_OK) return fail("rt_multi_create");
    std::vector<rt_scene *> scs(gpus, nullptr);
    std::vector<rt_material> mats(RT_REFERENCE_MATERIALS);
    std::vector<rt_light> lights(RT_REFERENCE_LIGHTS);
    rt_reference_materials(mats.data());
    rt_reference_lights(lights.data());
    std::string json;  // a scene description file (rt_scene_desc_parse), re-read at every frame's time
    if (scene.size() > 5 && scene.compare(scene.size() - 5, 5, ".json") == 0) {
        std::ifstream f(scene);
        if (!f) { std::fprintf(stderr, "rt_cli: cannot read %s\n", scene.c_str()); return 2; }
        std::stringstream ss;
        ss << f.rdbuf();
        json = ss.str();
    }
    std::vector<float> frame(static_cast<size_t>(width) * height * 4);
    for (int k = 0; k < frames; ++k) {
        const float t = time0 + k * dt;
        std::vector<rt_object> objs;
        rt_camera cam;
        int has_cam = 0;
        if (!json.empty()) {
            int no = 0, nm = 0, nl = 0;
            objs.resize(RT_MAX_OBJECTS);
            mats.resize(RT_MAX_MATERIALS);
            lights.resize(RT_MAX_LIGHTS);
            if (rt_scene_desc_parse(json.c_str(), t, objs.data(), RT_MAX_OBJECTS, &no, mats.data(), RT_MAX_MATERIALS,
                                    &nm, lights.data(), RT_MAX_LIGHTS, &nl, &cam, &has_cam) != RT_OK)
                return fail("rt_scene_desc_parse");
            objs.resize(no);
            mats.resize(nm);
            lights.resize(nl);
        } else if (scene == "shipped") {
            objs.resize(RT_REFERENCE_OBJECTS);
            rt_reference_objects(t, objs.data());
        } else if (scene.rfind("spheres:", 0) == 0) {
            int n = 0;
            unsigned long long seed = 0;
            std::sscanf(scene.c_str() + 8, "%d:%llu", &n, &seed);
            objs.resize(static_cast<size_t>(n) + 1);
            if (rt_bench_objects(n, seed, objs.data()) != RT_OK) return fail("rt_bench_objects");
        } else {
            std::fprintf(stderr, "rt_cli: unknown scene %s\n", scene.c_str());
            return 2;
        }
        for (int g = 0; g < gpus; ++g) {  // the frame's scene on every GPU
            if (!scs[g]) {
                if (rt_scene_create(ctxs[g], objs.data(), static_cast<int>(objs.size()), mats.data(),
                                    static_cast<int>(mats.size()), lights.data(), static_cast<int>(lights.size()),
                                    &scs[g]) != RT_OK)
                    return fail("rt_scene_create");
            } else if (rt_scene_update(ctxs[g], scs[g], objs.data(), static_cast<int>(objs.size()), mats.data(),
                                       static_cast<int>(mats.size()), lights.data(),
                                       static_cast<int>(lights.size())) != RT_OK) {
                return fail("rt_scene_update");
            }
        }
        const auto t0 = std::chrono::steady_clock::now();
        if (group) {
            if (rt_render_multi(group, scs.data(), has_cam ? &cam : nullptr, t, width, height, depth, block_rows,
                                frame.data(), 0) != RT_OK)
                return fail("rt_render_multi");
        } else if (aa_spp > 0) {
            if (rt_render_aa(ctx, scs[0], has_cam ? &cam : nullptr, t, width, height, depth, aa_spp, 0u, aa_threshold,
                             frame.data(), nullptr, 0, nullptr) != RT_OK)
                return fail("rt_render_aa");
        } else if (rt_render(ctx, scs[0], has_cam ? &cam : nullptr, t, width, height, depth, 0, height, frame.data(),
                             0, nullptr) != RT_OK) {
            return fail("rt_render");
        }
        const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (aa_spp > 0) {
            int64_t px = 0, tiles = 0;
            if (rt_aa_last_counts(ctx, &px, &tiles) != RT_OK) return fail("rt_aa_last_counts");
            std::printf("frame %d aa %d spp, threshold %g: %lld of %lld pixels supersampled, in %lld wave tiles\n", k,
                        aa_spp, aa_threshold, static_cast<long long>(px), static_cast<long long>(width) * height,
                        static_cast<long long>(tiles));
        }
        if (group) {
            std::vector<float> kms(gpus, 0.0f);
            float gms = 0.0f, ams = 0.0f;
            rt_multi_last_ms(group, kms.data(), &gms, &ams);
            std::printf("frame %d t=%.4f  kernels", k, t);
            for (float v : kms) std::printf(" %.3f", v);
            std::printf(" ms  gather %.3f ms  assembly %.3f ms  call %.3f ms (incl. device->host copy)\n", gms, ams,
                        wall * 1e3);
        } else {
            float kms = 0.0f;
            rt_last_kernel_ms(ctx, &kms);
            std::printf("frame %d t=%.4f  kernel %.3f ms  call %.3f ms (incl. device->host copy)\n", k, t, kms,
                        wall * 1e3);
        }
        if (!ppm.empty() && rt_write_ppm(frame_name(ppm, k).c_str(), frame.data(), width, height) != RT_OK)
            return fail("rt_write_ppm");
        if (!pfm.empty() && rt_write_pfm(frame_name(pfm, k).c_str(), frame.data(), width, height) != RT_OK)
            return fail("rt_write_pfm");
        if (!hits.empty()) {
            const size_t n_px = static_cast<size_t>(width) * height;
            std::vector<rt_hit> rec(n_px);
            std::vector<float> nrm(n_px * 4), pnt(n_px * 4), enc(n_px * 4);
            if (rt_render_hits(ctx, scs[0], has_cam ? &cam : nullptr, t, width, height, 0, height, RT_HITS_SHADOW,
                               rec.data(), nrm.data(), pnt.data(), 0, nullptr) != RT_OK)
                return fail("rt_render_hits");
            for (size_t i = 0; i < n_px; ++i) {  // (object, t, shadow mask) as floats
                enc[4 * i] = static_cast<float>(rec[i].object);
                enc[4 * i + 1] = rec[i].t;
                enc[4 * i + 2] = static_cast<float>(rec[i].shadow);
                enc[4 * i + 3] = 0.0f;
            }
            const std::string prefix = frame_name(hits, k);
            if (rt_write_pfm((prefix + ".hit.pfm").c_str(), enc.data(), width, height) != RT_OK ||
                rt_write_pfm((prefix + ".normal.pfm").c_str(), nrm.data(), width, height) != RT_OK ||
                rt_write_pfm((prefix + ".point.pfm").c_str(), pnt.data(), width, height) != RT_OK)
                return fail("rt_write_pfm");
        }
    }
    rt_multi_destroy(group);
    for (int g = 0; g < gpus; ++g) {
        rt_scene_destroy(scs[g]);
        rt_destroy(ctxs[g]);
    }
    return 0;
}
