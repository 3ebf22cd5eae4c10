/* render_gltf.c — the C ABI used the way bevy-strolle's `cornell` / `demo` examples use strolle::Engine
 * (bevy-strolle/examples/cornell.rs, demo.rs): load a scene, add a light, create a camera, tick + render a few frames,
 * write the last one as a binary PPM. Plain C99 on purpose: this file is also the proof that include/strolle_hip.h is a
 * C header.
 *
 *   cc -std=c99 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/render_gltf.c \
 *      -L strolle_amd/csrc -lstrolle_hip -L /opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,$PWD/strolle_amd/csrc -o render_gltf
 *   ./render_gltf scene.glb out.ppm [width height frames] [--env sky.hdr [intensity]]
 *                 [--tonemap none|reinhard|reinhard-lum|aces|neutral] [--exposure EV] [--auto-exposure] [--normal-maps]
 * --normal-maps turns normal mapping on (st_engine_set_normal_mapping): the materials' normalTexture bends the primary hits' normals.
 * --env lights the scene with an equirectangular Radiance .hdr map instead of the atmosphere (st_decode_hdr + st_environment_set).
 * --tonemap, --exposure and --auto-exposure set the camera's display transform (st_camera_set_display): without them the 8-bit output
 * clips every channel at 1, as before. With --auto-exposure, --exposure is the compensation in EV.
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "strolle_hip.h"

#define CHECK(call)                                                                 \
    do {                                                                            \
        int status_ = (call);                                                       \
        if (status_ != ST_OK) {                                                     \
            fprintf(stderr, "%s failed (%d): %s\n", #call, status_, st_last_error()); \
            return 1;                                                               \
        }                                                                           \
    } while (0)

/* glam::Mat4::look_at_rh inverted = camera-to-world, column-major (what Bevy's GlobalTransform::compute_matrix gives) */
static void camera_to_world(const float eye[3], const float target[3], float out[16]) {
    float f[3], r[3], u[3], n;
    int i;
    for (i = 0; i < 3; i++) f[i] = target[i] - eye[i];
    n = sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (i = 0; i < 3; i++) f[i] /= n;
    r[0] = -f[2]; r[1] = 0.0f; r[2] = f[0];          /* cross(f, +Y) */
    n = sqrtf(r[0] * r[0] + r[2] * r[2]);
    for (i = 0; i < 3; i++) r[i] /= n;
    u[0] = r[1] * f[2] - r[2] * f[1]; u[1] = r[2] * f[0] - r[0] * f[2]; u[2] = r[0] * f[1] - r[1] * f[0];
    memset(out, 0, 16 * sizeof(float));
    for (i = 0; i < 3; i++) { out[i] = r[i]; out[4 + i] = u[i]; out[8 + i] = -f[i]; out[12 + i] = eye[i]; }
    out[15] = 1.0f;
}

/* glam::Mat4::perspective_infinite_reverse_rh (Bevy's PerspectiveProjection), column-major */
static void perspective_infinite_reverse(float fov_y, float aspect, float z_near, float out[16]) {
    const float f = 1.0f / tanf(0.5f * fov_y);
    memset(out, 0, 16 * sizeof(float));
    out[0] = f / aspect; out[5] = f; out[11] = -1.0f; out[14] = z_near;
}

/* a Radiance .hdr file as the sky: decoded by the library, copied by st_environment_set, live from the next st_tick */
static int set_environment(StEngine* engine, const char* path, float intensity) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return 1; }
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char* bytes = (unsigned char*)malloc(size > 0 ? (size_t)size : 1u);
    const int read_ok = bytes && fread(bytes, 1, (size_t)size, f) == (size_t)size;
    fclose(f);
    if (!read_ok) { fprintf(stderr, "could not read %s\n", path); free(bytes); return 1; }
    uint32_t w = 0, h = 0;
    float* rgb = NULL;
    int status = st_decode_hdr(bytes, (size_t)size, NULL, 0, &w, &h);
    if (status == ST_OK) {
        rgb = (float*)malloc((size_t)w * h * 3u * sizeof(float));
        status = rgb ? st_decode_hdr(bytes, (size_t)size, rgb, (size_t)w * h * 3u, &w, &h) : ST_ERR_INVALID_ARGUMENT;
    }
    if (status == ST_OK) {
        StEnvironmentDesc desc;
        memset(&desc, 0, sizeof desc);
        desc.struct_size = sizeof desc; desc.intensity = intensity;
        status = st_environment_set(engine, rgb, w, h, 3, &desc);
    }
    if (status != ST_OK) fprintf(stderr, "environment %s failed (%d): %s\n", path, status, st_last_error());
    else fprintf(stderr, "environment %s: %ux%u, intensity %g\n", path, w, h, intensity);
    free(rgb); free(bytes);
    return status != ST_OK;
}

int main(int argc, char** argv) {
    const char* env_path = NULL;
    float env_intensity = 1.0f;
    const char* pos[5] = {NULL, NULL, NULL, NULL, NULL};
    const char* tonemap_names[5] = {"none", "reinhard", "reinhard-lum", "aces", "neutral"};
    int npos = 0, i, display = 0, tonemap = ST_TONEMAP_NONE, auto_exposure = 0, normal_maps = 0;
    float exposure_ev = 0.0f;
    for (i = 1; i < argc; i++) {
        if (strcmp(argv[i], "--tonemap") == 0 && i + 1 < argc) {
            int k, found = 0;
            ++i;
            for (k = 0; k < 5; k++) if (strcmp(argv[i], tonemap_names[k]) == 0) { tonemap = k; found = 1; }
            if (!found) { fprintf(stderr, "unknown tonemap %s\n", argv[i]); return 2; }
            display = 1;
        } else if (strcmp(argv[i], "--exposure") == 0 && i + 1 < argc) {
            exposure_ev = strtof(argv[++i], NULL); display = 1;
        } else if (strcmp(argv[i], "--auto-exposure") == 0) {
            auto_exposure = 1; display = 1;
        } else if (strcmp(argv[i], "--normal-maps") == 0) {
            normal_maps = 1;
        } else if (strcmp(argv[i], "--env") == 0 && i + 1 < argc) {
            env_path = argv[++i];
            if (i + 1 < argc) { char* end; const float v = strtof(argv[i + 1], &end); if (end != argv[i + 1] && *end == '\0') { env_intensity = v; i++; } }
        } else if (npos < 5) pos[npos++] = argv[i];
    }
    if (npos < 2) {
        fprintf(stderr, "usage: %s scene.gltf|scene.glb out.ppm [width height frames] [--env sky.hdr [intensity]] "
                        "[--tonemap none|reinhard|reinhard-lum|aces|neutral] [--exposure EV] [--auto-exposure] [--normal-maps]\n", argv[0]);
        return 2;
    }
    const uint32_t width = npos > 2 ? (uint32_t)atoi(pos[2]) : 640u, height = npos > 3 ? (uint32_t)atoi(pos[3]) : 360u;
    const int frames = npos > 4 ? atoi(pos[4]) : 24;

    StEngine* engine = NULL;
    CHECK(st_engine_create(0, &engine));
    if (normal_maps) CHECK(st_engine_set_normal_mapping(engine, 1));                    /* off by default: the picture without the flag is unchanged */

    StGltfOptions options;
    memset(&options, 0, sizeof options);
    options.first_handle = 1; options.first_image_handle = 1000;
    options.light_radius = 0.15f;                                                       /* cornell.rs:45-54 */
    StGltfSummary scene;
    CHECK(st_scene_load_gltf(engine, pos[0], &options, &scene));
    fprintf(stderr, "%u meshes, %u triangles, %u materials, %u images (%u dropped, %u primitives skipped), %u lights\n", scene.meshes,
            scene.triangles, scene.materials, scene.images, scene.images_dropped, scene.primitives_skipped, scene.lights);

    StLight light;                                                                      /* the example's own lamp, on top of the file's */
    memset(&light, 0, sizeof light);
    light.kind = ST_LIGHT_POINT;
    light.position[0] = 0.0f; light.position[1] = 1.5f; light.position[2] = 0.5f;
    light.radius = 0.15f; light.range = 35.0f;
    light.color[0] = light.color[1] = light.color[2] = 50.0f / (4.0f * 3.14159265f);   /* cornell.rs:45-54 */
    CHECK(st_light_insert(engine, 1 + scene.lights, &light));
    CHECK(st_sun_update(engine, 0.0f, -1.0f));                                          /* night: cornell.rs:87 */
    if (env_path && set_environment(engine, env_path, env_intensity)) return 1;

    StCamera camera;
    memset(&camera, 0, sizeof camera);
    camera.mode = ST_MODE_IMAGE; camera.denoise = 1; camera.width = width; camera.height = height;
    {
        const float eye[3] = {0.0f, 1.0f, 3.2f}, target[3] = {0.0f, 1.0f, 0.0f};          /* cornell.rs:76-78 */
        camera_to_world(eye, target, camera.transform);
        perspective_infinite_reverse(3.14159265f / 4.0f, (float)width / (float)height, 0.1f, camera.projection);
    }
    StHandle cam = 0;
    CHECK(st_camera_create(engine, &camera, &cam));
    CHECK(st_camera_set_output_format(engine, cam, ST_FORMAT_RGBA8_UNORM_SRGB));        /* what a swap chain would hold */
    if (display) {                                                                      /* exposure + tone mapping before the 8-bit store */
        StDisplayDesc d;
        memset(&d, 0, sizeof d);
        d.struct_size = sizeof d; d.tonemap = (uint32_t)tonemap; d.exposure_ev = exposure_ev;
        d.flags = auto_exposure ? ST_DISPLAY_AUTO_EXPOSURE : 0u;
        d.ev_min = -12.0f; d.ev_max = 8.0f; d.low_fraction = 0.1f; d.high_fraction = 0.9f;   /* the metering range and the ranks kept */
        d.max_ev_step_up = 1.0f; d.max_ev_step_down = 1.0f;                                   /* adaptation: 1 EV per frame at most */
        CHECK(st_camera_set_display(engine, cam, &d));
        fprintf(stderr, "display: tonemap %s, %s exposure %g EV\n", tonemap_names[tonemap], auto_exposure ? "auto," : "manual", exposure_ev);
    }

    /* The present path of the Rust facade (rust/strolle-hip/src/present.rs), in C: two device frames and two page-locked
     * host frames alternate; frame N's copy to the host is enqueued behind its composition and runs while frame N+1
     * renders, and what gets presented at tick N+1 is frame N (one frame of latency, no stream synchronisation). */
    const size_t frame_bytes = (size_t)width * height * 4;
    void* frame[2] = {NULL, NULL};
    void* host_frame[2] = {NULL, NULL};
    for (int k = 0; k < 2; k++)
        if (hipMalloc(&frame[k], frame_bytes) != hipSuccess || hipHostMalloc(&host_frame[k], frame_bytes, 0) != hipSuccess) { fprintf(stderr, "allocation failed\n"); return 1; }
    unsigned char* host = (unsigned char*)malloc(frame_bytes);   /* stands in for queue.write_texture's destination */
    if (!host) return 1;
    int presented = 0, waited = 0;
    for (int i = 0; i < frames; i++) {        /* the loop of bevy-strolle's render node: update_camera, tick, render_camera */
        const int k = i & 1;
        CHECK(st_camera_update(engine, cam, &camera));
        CHECK(st_tick(engine, NULL));
        CHECK(st_render_camera(engine, cam, frame[k], NULL));
        CHECK(st_camera_present_copy(engine, cam, frame[k], host_frame[k], frame_bytes, NULL));
        if (i > 0) {                          /* present frame i-1: its copy was enqueued a whole frame ago */
            int ready = 0;
            CHECK(st_camera_present_ready(engine, cam, host_frame[k ^ 1], 0, &ready));
            if (!ready) { waited++; CHECK(st_camera_present_ready(engine, cam, host_frame[k ^ 1], 1, &ready)); }
            memcpy(host, host_frame[k ^ 1], frame_bytes);
            presented++;
        }
    }
    {                                         /* the last frame */
        int ready = 0;
        CHECK(st_camera_present_ready(engine, cam, host_frame[(frames - 1) & 1], 1, &ready));
        memcpy(host, host_frame[(frames - 1) & 1], frame_bytes);
        presented++;
    }
    uint64_t rays = 0;
    CHECK(st_camera_ray_count(engine, cam, &rays, 0));

    FILE* f = fopen(pos[1], "wb");
    if (!f) { perror(pos[1]); return 1; }
    fprintf(f, "P6\n%u %u\n255\n", width, height);
    for (size_t i = 0; i < (size_t)width * height; i++) fwrite(host + 4 * i, 1, 3, f);
    fclose(f);
    fprintf(stderr, "%d frames (%d presented, %d waited for their copy), %llu rays, wrote %s\n", frames, presented, waited, (unsigned long long)rays, pos[1]);

    free(host);
    for (int k = 0; k < 2; k++) { (void)hipFree(frame[k]); (void)hipHostFree(host_frame[k]); }
    CHECK(st_camera_delete(engine, cam));
    st_engine_destroy(engine);
    return 0;
}
