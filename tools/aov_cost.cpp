// Cost of the first-hit feature buffers (surf_read_aov) against the path a
// caller had before them: per-pixel camera rays built on the host, pushed
// through surf_trace_closest (two ray uploads, k_trace_closest, the hit
// records back) -- what classifyPixels does privately for the issue order.
// Bundled indoor scene, one MI355X; per frame size, `reps` fresh contexts:
//   aov_kernel_ms   k_aov, HIP events on the render stream (surf_debug_aov_time)
//   aov_first_ms    first surf_read_aov(SURF_AOV_ID): plane allocation, kernel, one plane back
//   aov_cached_ms   a second read (the copy alone)
//   rays_host_ms    the host loop that builds the rays (classifyPixels' loop)
//   trace_call_ms   surf_trace_closest of those rays (its host-side unpacking included)
// and checks that both paths name the same instance and primitive per pixel.
// Kernel times of k_trace_closest come from a kernel trace of this program.
// build: g++ -O3 -std=c++17 -Iinclude tools/aov_cost.cpp -o tools/aov_cost
//            -Lsurf-path-tracer_amd/lib -lsurf_hip -Wl,-rpath,'$ORIGIN/../surf-path-tracer_amd/lib'
// usage: tools/aov_cost ASSETS_DIR [reps]
#include "surf_hip.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static double msSince(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
#define OK(call) do { const int rc_ = (call); if (rc_ != SURF_OK) { std::fprintf(stderr, "%s: %d %s\n", #call, rc_, surf_last_error(nullptr)); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s ASSETS_DIR [reps]\n", argv[0]); return 2; }
    const int reps = argc > 2 ? std::atoi(argv[2]) : 5;
    surf_scene* scene = nullptr;
    OK(surf_scene_build_indoor(argv[1], 0, &scene));
    surf_scene_desc desc;
    OK(surf_scene_desc_get(scene, &desc));
    const uint32_t sizes[2][2] = {{1280, 720}, {1920, 1080}};
    for (const auto& wh : sizes) {
        const uint32_t W = wh[0], H = wh[1], n = W * H;
        surf_camera_ubo cam;
        OK(surf_scene_camera(scene, W, H, &cam));
        for (int rep = 0; rep < reps; ++rep) {
            surf_ctx* c = nullptr;
            OK(surf_create(0, W, H, 0, H, &c));
            OK(surf_upload_scene(c, &desc));
            OK(surf_set_camera(c, &cam));
            std::vector<uint32_t> ids(4 * (size_t)n);
            auto t0 = std::chrono::steady_clock::now();
            OK(surf_read_aov(c, SURF_AOV_ID, ids.data()));
            const double aovFirst = msSince(t0);
            float aovKernel = 0.0f;
            OK(surf_debug_aov_time(c, &aovKernel));
            t0 = std::chrono::steady_clock::now();
            OK(surf_read_aov(c, SURF_AOV_ID, ids.data()));
            const double aovCached = msSince(t0);

            t0 = std::chrono::steady_clock::now();
            std::vector<float> o(3 * (size_t)n), d(3 * (size_t)n);
            const float pos[3] = {cam.position.x, cam.position.y, cam.position.z};
            const float fp[3] = {cam.first_pixel.x, cam.first_pixel.y, cam.first_pixel.z};
            const float uv[3] = {cam.u_vector.x, cam.u_vector.y, cam.u_vector.z};
            const float vv[3] = {cam.v_vector.x, cam.v_vector.y, cam.v_vector.z};
            const float invW = 1.0f / cam.resolution[0], invH = 1.0f / cam.resolution[1];
            for (uint32_t lp = 0; lp < n; ++lp) {
                const float u = (float)(lp % W) * invW, v = (float)(lp / W) * invH;
                float dir[3], len2 = 0.0f;
                for (int a = 0; a < 3; ++a) {
                    dir[a] = fp[a] + u * uv[a] + v * vv[a] - pos[a];
                    len2 += dir[a] * dir[a];
                }
                const float inv = 1.0f / std::sqrt(len2);
                for (int a = 0; a < 3; ++a) { o[3 * (size_t)lp + a] = pos[a]; d[3 * (size_t)lp + a] = dir[a] * inv; }
            }
            const double raysHost = msSince(t0);
            std::vector<float> t(n), hu(n), hv(n);
            std::vector<uint32_t> inst(n), prim(n);
            t0 = std::chrono::steady_clock::now();
            OK(surf_trace_closest(c, n, o.data(), d.data(), t.data(), hu.data(), hv.data(), inst.data(), prim.data()));
            const double traceCall = msSince(t0);
            size_t differ = 0;
            for (uint32_t p = 0; p < n; ++p) differ += ids[4 * (size_t)p] != inst[p] || ids[4 * (size_t)p + 1] != prim[p];
            std::printf("{\"width\": %u, \"height\": %u, \"rep\": %d, \"aov_kernel_ms\": %.4f, \"aov_first_ms\": %.3f, \"aov_cached_ms\": %.3f, "
                        "\"rays_host_ms\": %.3f, \"trace_call_ms\": %.3f, \"ids_differ\": %zu}\n",
                        W, H, rep, aovKernel, aovFirst, aovCached, raysHost, traceCall, differ);
            std::fflush(stdout);
            surf_destroy(c);
            if (differ) return 1;
        }
    }
    surf_scene_destroy(scene);
    return 0;
}
