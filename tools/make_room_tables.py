"""Room tables for b32_room_hover / b32_room_box_select from the reference's OWN sample levels.  BUILD CONTAINER ONLY: it reads the
reference's assets (through load_level of tools/make_real_scenes.py) and writes DATA -- tests/golden/rooms/<level>-room0.npz: the room's
sector faces as abi.SECTOR_FACE_DTYPE records in iter_sectors order (room_faces_from_sectors), its grid, and the camera and framebuffer
size of the matching golden room scene under tests/golden/scenes/real/.  Only those files travel; nothing of the reference's text is
copied.

usage: python tools/make_room_tables.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bonnie32_amd as b32                       # noqa: E402
from bonnie32_amd import scenefile               # noqa: E402
from make_real_scenes import load_level          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rooms")
SCENES = os.path.join(ROOT, "tests", "golden", "scenes", "real")
# level, room, the golden scene whose camera looks into that room
ROOMS = (("Dungeon", 0, "dungeon-room0-game"), ("Cave", 0, "cave-room0-game"), ("Cathedral", 0, "cathedral-room0-game-640"),
         ("Sewers", 0, "sewers-room0-painter"))


def main():
    os.makedirs(OUT, exist_ok=True)
    for level, idx, scene in ROOMS:
        room = load_level(level)["rooms"][idx]
        faces = b32.room_faces_from_sectors(room["sectors"])
        grid = np.zeros(1, b32.abi.ROOM_GRID_DTYPE)
        grid["position"][0] = [room["position"][k] for k in "xyz"]
        grid["sector_size"] = b32.abi.SECTOR_SIZE
        sc = scenefile.read_scene(os.path.join(SCENES, scene + ".b32scene"))
        cam = np.array([sc.camera.position, sc.camera.basis_x, sc.camera.basis_y, sc.camera.basis_z], np.float32)
        path = os.path.join(OUT, f"{level.lower()}-room{idx}.npz")
        np.savez(path, faces=faces, grid=grid, camera=cam, size=np.array([sc.width, sc.height], np.uint32))
        kinds = np.bincount(faces["kind"], minlength=8)
        print(f"{os.path.basename(path):24s} {len(faces):5d} records  kinds {kinds.tolist()}  {sc.width}x{sc.height}  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
