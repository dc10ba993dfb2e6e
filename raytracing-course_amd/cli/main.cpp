// pt_render -- drop-in for the reference CLI (hw5/src/main.cpp:6-17, hw5/run.sh:1-2):
//     pt_render <scene.txt> <out.ppm>
// Load -> InitScene -> Render -> P6 file, on the GPU(s).  Optional environment:
//     PT_NGPU=<n>     GPUs driven by this process (pixel tiles, default 1)
//     PT_DEVICE=<i>   first device (default 0)
//     PT_SPP_LAUNCH=<k> samples per kernel launch (default auto)
//     PT_GATHER=rccl|host  framebuffer gather (default: RCCL when PT_NGPU > 1)
//     PT_QUIET=1      no progress bar
//     PT_FILTER=<levels>  write the image from the guided filter of the radiance (1..8 levels, the
//                     other options at their defaults; unset or 0: the render's own image)
//     PT_STATS=1      print rays / Mray/s / timings to stderr (2: also the phase times)
//     PT_FULL_EXIT=1  tear the scene and the HIP runtime down before exiting (default: the
//                     process leaves right after the PPM is closed; rocprofv3 needs the full exit)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <chrono>
#include <thread>
#include <vector>

#include "pt.h"

static int env_int(const char* k, int def) {
    const char* v = getenv(k);
    return v && *v ? atoi(v) : def;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s <scene.txt> <out.ppm>\n", argv[0]);
        return 2;
    }
    const auto t_main = std::chrono::steady_clock::now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_main).count(); };
    const int ngpu = env_int("PT_NGPU", 1), dev0 = env_int("PT_DEVICE", 0);
    double t_warm = 0, t_comm = 0, t_load = 0, t_join = 0, t_render = 0, t_write = 0;
    const char* gather = getenv("PT_GATHER");
    const bool host_gather = gather && !strcmp(gather, "host");
    // the HIP runtime starts on a second thread while the scene is parsed and its
    // BVH built, and with several GPUs the RCCL communicator of the framebuffer
    // gather is created there too (errors surface again, from pt_render)
    std::thread warm([&] {
        // one thread per device: each device's runtime context and code objects at once
        std::vector<std::thread> di;
        for (int g = 0; g < ngpu; ++g) di.emplace_back([g, dev0] { (void)pt_device_init(dev0 + g); });
        for (auto& t : di) t.join();
        t_warm = ms();
        if (ngpu > 1 && !host_gather) (void)pt_gather_init(dev0, ngpu);
        t_comm = ms();
    });
    pt_scene* s = nullptr;
    const bool ok = pt_scene_load(argv[1], &s) == PT_OK && pt_scene_prepare(s) == PT_OK;
    t_load = ms();
    warm.join();
    t_join = ms();
    if (!ok) {
        fprintf(stderr, "pt_render: %s\n", pt_last_error());
        pt_scene_free(s);
        return 1;
    }
    pt_scene_info info;
    pt_scene_get_info(s, &info);
    pt_render_opts o;
    pt_render_opts_default(&o);
    o.ngpu = ngpu;
    o.device = dev0;
    o.spp_per_launch = (uint32_t)env_int("PT_SPP_LAUNCH", 0);
    o.progress = env_int("PT_QUIET", 0) ? 0 : 1;
    if (gather) {
        if (!strcmp(gather, "rccl")) o.gather = PT_GATHER_RCCL;
        else if (host_gather) o.gather = PT_GATHER_HOST;
    }
    std::vector<uint8_t> rgb((size_t)info.width * info.height * 3);
    pt_stats st;
    // PT_FILTER=<levels>: the render's radiance through the guided filter, the image from its 8-bit form
    const int filter_levels = env_int("PT_FILTER", 0);
    std::vector<float> rad(filter_levels ? rgb.size() : 0);
    if (pt_render(s, &o, rgb.data(), filter_levels ? rad.data() : nullptr, &st) != PT_OK) {
        fprintf(stderr, "pt_render: %s\n", pt_last_error());
        pt_scene_free(s);
        return 1;
    }
    if (filter_levels) {
        pt_filter_opts fo;
        pt_filter_opts_default(&fo);
        fo.levels = (uint32_t)filter_levels;   // (outside 1..8: the library's refusal)
        std::vector<float> out(rad.size());
        if (pt_filter(s, dev0, 0, 0, 0, 0, &fo, rad.data(), out.data(), rgb.data()) != PT_OK) {
            fprintf(stderr, "pt_render: %s\n", pt_last_error());
            pt_scene_free(s);
            return 1;
        }
    }
    t_render = ms();
    if (pt_write_ppm(argv[2], info.width, info.height, rgb.data()) != PT_OK) {
        fprintf(stderr, "pt_render: %s\n", pt_last_error());
        pt_scene_free(s);
        return 1;
    }
    t_write = ms();
    if (env_int("PT_STATS", 0) >= 2) {
        fprintf(stderr, "phases_ms: device_init=%.1f comm_init=%.1f load_prepare=%.1f join=%.1f render=%.1f write=%.1f\n",
                t_warm, t_comm, t_load, t_join, t_render, t_write);
        // wall-clock stamps of main()'s start and of the PPM closed (the caller's clock brackets
        // process start-up before main and the exit after it)
        const double unix_now = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
        fprintf(stderr, "unix_main=%.6f unix_written=%.6f\n", unix_now - ms() / 1e3, unix_now);
    }
    if (env_int("PT_STATS", 0)) {
        fprintf(stderr, "rays=%llu samples=%llu kernel_ms=%.3f wall_ms=%.3f Mray/s=%.3f ngpu=%d gather_rccl=%llu "
                "fallbacks=%llu rounds=%llu\n",
                (unsigned long long)st.rays, (unsigned long long)st.samples, st.kernel_ms, st.wall_ms,
                st.kernel_ms > 0 ? st.rays / (st.kernel_ms * 1e3) : 0.0, ngpu, (unsigned long long)st.gather_rccl,
                (unsigned long long)st.fallbacks, (unsigned long long)st.rounds);
    }
    // The PPM is written and closed: leave without tearing down the scene's device
    // memory and the HIP runtime one by one (the process exit releases them; the
    // teardown only adds to the wall-clock of `run.sh`)
    // (PT_FULL_EXIT=1 keeps the normal exit: tools that flush at exit, e.g. rocprofv3)
    if (env_int("PT_FULL_EXIT", 0)) {
        pt_scene_free(s);
        return 0;
    }
    fflush(stdout);
    fflush(stderr);
    _exit(0);
}
