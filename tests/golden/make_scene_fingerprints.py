#!/usr/bin/env python3
"""Regenerates tests/golden/scene_fingerprints.json from the benchmark scenes' original files (run from the repo root):

    python tests/golden/make_scene_fingerprints.py <directory holding bevy-strolle's cornell.zip and demo.zip>

The originals are not part of this repository; assets/*.npz were converted from them by tools/convert_assets.py. For each
scene the glTF loader reads the original file and the digests of the resulting engine state (tests/parity.py scene_fingerprint)
and of every decoded texture are written. Before anything is written, the committed conversion inserted through the Python API
has to give the same engine state bit for bit (BVH stream included): the fingerprints pin the conversions to the real scenes."""
import hashlib
import json
import os
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from parity import assert_bits_equal, scene_fingerprint  # noqa: E402
from strolle_amd import Engine, scenes  # noqa: E402
from strolle_amd.api import decode_png  # noqa: E402

# name -> (archive, file inside it, npz, load_gltf keywords, material overrides of the API route)
SCENES = {
    "cornell": ("cornell.zip", "cornell/scene.gltf", "cornell.npz", {}, None),
    "dungeon": ("demo.zip", "demo/level.glb", "dungeon.npz", dict(reflectance=0.0, perceptual_roughness=1.0), dict(reflectance=0.0, perceptual_roughness=1.0)),
    "dungeon-subdivided": ("demo.zip", "demo/level.glb", "dungeon.npz", dict(reflectance=0.0, perceptual_roughness=1.0, subdivide=1), dict(reflectance=0.0, perceptual_roughness=1.0)),
}


def glb_pngs(path):
    glb = open(path, "rb").read()
    n = np.frombuffer(glb[12:16], "<u4")[0]
    doc = json.loads(glb[20:20 + n])
    binary = glb[20 + n + 8:]
    out = []
    for image in doc["images"]:
        view = doc["bufferViews"][image["bufferView"]]
        out.append(binary[view.get("byteOffset", 0): view.get("byteOffset", 0) + view["byteLength"]])
    return out


def main(src):
    result = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (archive, inner, npz, kw, overrides) in SCENES.items():
            zipfile.ZipFile(os.path.join(src, archive)).extractall(tmp)
            path = os.path.join(tmp, inner)
            converted = np.load(os.path.join(scenes.ASSETS, npz))
            a, b = Engine(device=-1), Engine(device=-1)
            summary = a.load_gltf(path, **kw)
            scenes._insert_gltf(b, converted, material_overrides=overrides, subdivide=kw.get("subdivide", 0))
            for e in (a, b):
                e.tick()
            for what, label in enumerate(("BVH stream", "triangles", "lights", "materials")):
                assert_bits_equal(a.read_scene(what), b.read_scene(what), f"{name}: {label}")
            entry = {"source": f"{archive}:{inner}", "meshes": summary["meshes"], "images": summary["images"], **scene_fingerprint(a, summary["triangles"])}
            if path.endswith(".glb"):
                texels = [decode_png(png) for png in glb_pngs(path)]
                for i, t in enumerate(texels):
                    assert np.array_equal(t, converted[f"image_{i}"]), f"{name}: texture {i}"
                entry["textures_sha256"] = [hashlib.sha256(np.ascontiguousarray(t, np.uint8).tobytes()).hexdigest() for t in texels]
            result[name] = entry
            a.close(); b.close()
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scene_fingerprints.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv[1])
