"""Material tables for b32_room_build_mesh from the reference's OWN sample levels.  BUILD CONTAINER ONLY: it reads the reference's assets
(through load_level / level_textures of tools/make_real_scenes.py) and writes DATA -- tests/golden/rooms/<level>-room0.materials.npz: one
abi.FACE_MATERIAL_DTYPE record per record of <level>-room0.npz (room_materials_from_sectors), with room_scene's resolve and its only_used
texture remap, so that the texture ids are those of the golden room scenes under tests/golden/scenes/real/.  Only those files travel;
nothing of the reference's text is copied.

usage: python tools/make_room_materials.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bonnie32_amd as b32                                   # noqa: E402
from make_real_scenes import level_textures, load_level      # noqa: E402
from make_room_tables import OUT, ROOMS                      # noqa: E402


def main():
    for level_name, idx, _scene in ROOMS:
        level = load_level(level_name)
        texs, names = level_textures(level)
        room = level["rooms"][idx]

        def resolve(ref):                                    # game/renderer.rs:104-112, as room_scene states it
            if not ref or not ref.get("name"):
                return None
            for i, n in enumerate(names):
                if n == ref["name"]:
                    return i, texs[i].width
            return None
        faces = b32.room_faces_from_sectors(room["sectors"])
        mats = b32.room_materials_from_sectors(room["sectors"], resolve)
        flat = faces["kind"] < 2
        used = sorted(set(mats["texture_id"].tolist()) | set(mats["texture_id_2"][flat].tolist()))     # room_scene's only_used remap
        remap = np.zeros(max(used) + 1, np.uint32)
        remap[used] = np.arange(len(used), dtype=np.uint32)
        mats["texture_id"] = remap[mats["texture_id"]]; mats["texture_id_2"] = remap[mats["texture_id_2"]]
        path = os.path.join(OUT, f"{level_name.lower()}-room{idx}.materials.npz")
        np.savez_compressed(path, materials=mats)
        nv, nf = b32.room_mesh_counts(faces, mats)
        print(f"{os.path.basename(path):34s} {len(mats):5d} records  {nv} vertices  {nf} faces  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
