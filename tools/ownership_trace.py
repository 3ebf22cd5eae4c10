"""One fixed sequence of ABI calls for comparing the HIP calls two builds of the library issue (STROLLE_HIP_LIB picks the library):
Cornell, then the dungeon, 1920 x 1080 Image{denoise}, 30 frames each with one spawn, one light move and one re-pose (a skinned tube,
deformation motion on) in between, an environment map set and replaced, a look-up table (colour grading on) inserted and replaced, auto-exposure
display and FXAA + resize for the last 10, a second stream alternating with the first for the last 5 (mixed streams: the light moves back and the
map and the table are replaced once more there, so that the writer and both retirements join the device), then st_camera_delete and st_engine_destroy.
The scene stores' paths too: an image inserted and later replaced at another size, a material edited to point at it, the spawned instance removed, one
static and one dynamic device image.
Run it under `rocprofv3 --hip-trace --stats -- python tools/ownership_trace.py` once per library; with --summarize DIR it prints the
per-API call counts of the trace under DIR as one JSON object."""
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarize(directory):
    files = glob.glob(os.path.join(directory, "**", "*hip_api_stats.csv"), recursive=True)
    assert len(files) == 1, files
    print(json.dumps({r["Name"]: int(r["Calls"]) for r in csv.DictReader(open(files[0]))}, sort_keys=True))


def run():
    import numpy as np
    import torch
    from strolle_amd import CameraMode, Engine, Instance, Light, Material, Tonemap, scenes

    size, out_size, tube = (1920, 1080), (2560, 1440), 7000
    out = torch.zeros((out_size[1] * out_size[0], 4), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    mesh, joints, weights = scenes.skinned_tube(24, 12, 6, length=1.2)
    places = {"cornell": ((-0.4, 0.0, 0.0), (0.4, 0.0, -0.3), (0.0, 1.2, 1.0)), "dungeon": ((-6.1, 0.0, -19.0), (-5.4, 0.0, -19.0), (-5.75, 0.8, -18.0))}
    other = torch.cuda.Stream().cuda_stream
    sky = lambda seed: (np.random.default_rng(seed).random((8, 16, 3)) * 2.0).astype(np.float32)
    lut = lambda seed: np.random.default_rng(seed).random((5, 5, 5, 3)).astype(np.float32)
    at = lambda p: np.array([[1, 0, 0, p[0]], [0, 1, 0, p[1]], [0, 0, 1, p[2]]], np.float32)
    texels = lambda side, seed: np.random.default_rng(seed).integers(0, 256, (side, side, 4), dtype=np.uint8)
    static_px, dynamic_px = (torch.full((32, 32, 4), v, dtype=torch.uint8, device="cuda:0") for v in (90, 160))
    for scene in ("cornell", "dungeon"):
        e = Engine(device=0)
        (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(e)
        e.set_seed(7)
        first, second, lamp = places[scene]
        e.insert_material(tube, Material(base_color=(0.2, 0.7, 0.3, 1.0)))
        e.insert_mesh(tube, mesh); e.set_skin(tube, joints, weights, 6)
        e.insert_instance(tube, Instance(tube, tube, at(first)))
        e.insert_light(900, Light.point(lamp, 0.1, (2.0,) * 3, 20.0))
        e.set_deformation_motion(True)
        e.set_pose(tube, scenes.bend_pose(6, 1.6, 0.0, length=1.2))
        cam = e.create_camera((scenes.cornell_camera if scene == "cornell" else scenes.dungeon_camera)(size, CameraMode.IMAGE, denoise=True))
        e.insert_lut(41, lut(1)); e.set_color_grading(cam, lut=41, contrast=1.2)         # the table inserted
        for frame in range(30):
            if frame == 2:
                e.insert_image(5001, texels(48, 1))                                          # an image inserted
                e.insert_device_image(5002, static_px.data_ptr(), 32, 32)                    # a static device image
                e.insert_device_image(5003, dynamic_px.data_ptr(), 32, 32, dynamic=True)     # ... and a dynamic one
            if frame == 6:
                e.insert_image(5001, texels(96, 2))                                          # ... and replaced at another size
            if frame == 18:
                e.insert_material(tube, Material(base_color=(0.7, 0.3, 0.2, 1.0), base_color_texture=5001))   # the material edit
            if frame == 22:
                e.remove_instance(tube + 1)                                                  # the instance removed
            if frame == 4:
                e.set_environment(sky(1))                                                    # the map set
            if frame in (10, 27):
                e.set_environment(sky(frame))                                                # ... and replaced
            if frame in (14, 27):
                e.insert_lut(41, lut(frame))                                                 # the table replaced
            if frame == 27:
                e.insert_light(900, Light.point(lamp, 0.1, (2.0,) * 3, 20.0))
            if frame == 8:
                e.insert_instance(tube + 1, Instance(tube, tube, at(second)))                       # the spawn
            if frame == 12:
                e.insert_light(900, Light.point((lamp[0] + 0.2, lamp[1], lamp[2]), 0.1, (2.0,) * 3, 20.0))   # the light move
            if frame == 16:
                e.set_pose(tube, scenes.bend_pose(6, 1.6, 0.7, length=1.2))                         # the re-pose
            if frame == 20:
                e.set_display(cam, tonemap=Tonemap.ACES_FITTED, auto_exposure=True)
                e.set_post(cam, fxaa=True, output_size=out_size)
            s = other if frame >= 25 and frame % 2 else stream
            e.tick(s)
            e.render_camera(cam, out.data_ptr(), s)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        e.delete_camera(cam)
        e.close()


if __name__ == "__main__":
    summarize(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--summarize" else run()
