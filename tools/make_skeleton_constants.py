#!/usr/bin/env python3
"""Writes tests/golden/skeleton_constants.json: the literals the bone octahedra and the skeleton overlay rest on, read from the
reference's text (modeler/skeleton.rs, modeler/state.rs).  Data only: names and numbers.

    python tools/make_skeleton_constants.py <reference source tree>
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "skeleton_constants.json")


def one(pattern, text, what):
    m = re.search(pattern, text, re.S)
    if not m:
        raise SystemExit(f"make_skeleton_constants: {what} not found")
    return m


def rgb(m, first=1):
    return [int(m.group(first + k)) for k in range(3)]


def main(src):
    sk = open(os.path.join(src, "modeler", "skeleton.rs")).read()
    st = open(os.path.join(src, "modeler", "state.rs")).read()
    new = r"RasterColor::new\((\d+),\s*(\d+),\s*(\d+)\)"
    out = {"bone_colours": {}, "dots": {}}
    for name in ("default", "selected", "hovered", "tip_hovered", "root", "creating", "hierarchy_line"):
        out["bone_colours"][name] = rgb(one(r"fn bone_color_%s\(\) -> RasterColor \{\s*" % name + new, sk, name))
    dots = sk[sk.index("pub fn draw_bone_dots"):sk.index("fn draw_bone_octahedron")]
    named = {n: rgb(one(r"let %s = " % n + new, dots, n)) for n in ("tip_color", "tip_selected_color", "tip_hovered_color", "base_color")}
    named["bone_color_hovered()"] = out["bone_colours"]["hovered"]
    tip, base = dots[dots.index("// Draw tip dot"):dots.index("// Draw base dot")], dots[dots.index("// Draw base dot"):]
    for part, text, keys in (("tip", tip, ("tip_hovered", "tip_selected", "tip")), ("base", base, ("base_hovered", "base_selected", "base"))):
        pairs = re.findall(r"\((\d+),\s*([a-z_]+(?:\(\))?)\)", text)
        if len(pairs) != 3:
            raise SystemExit(f"make_skeleton_constants: the {part} dot's three (radius, colour) pairs not found")
        for key, (radius, colour) in zip(keys, pairs):
            out["dots"][key] = {"radius": int(radius), "colour": named[colour]}
    order = [w for _, w in sorted((dots.index("// Draw %s dot" % w), w) for w in ("tip", "base"))]
    out["dot_order"] = order
    out["dim_alpha"] = int(one(r"let dim_alpha: u8 = (\d+);", sk, "dim_alpha").group(1))
    out["default_width"] = float(one(r"pub const DEFAULT_WIDTH: f32 = ([0-9.]+);", st, "DEFAULT_WIDTH").group(1))
    gen = sk[sk.index("fn generate_bone_octahedron"):]
    out["degenerate_length"] = float(one(r"if length < ([0-9.]+) \{", gen, "the degenerate length").group(1))
    out["up_limit"] = float(one(r"dir\.y\.abs\(\) < ([0-9.]+)", sk, "the up limit").group(1))
    out["ring_at"] = float(one(r"dir_norm \* \(length \* ([0-9.]+)\)", gen, "the ring position").group(1))
    m = one(r"if self\.width > 0\.0 \{\s*self\.width\s*\} else \{\s*\(self\.length \* ([0-9.]+)\)\.clamp\(([0-9.]+), ([0-9.]+)\)", st, "display_width")
    out["display_width"] = {"scale": float(m.group(1)), "min": float(m.group(2)), "max": float(m.group(3))}
    body = one(r"pub fn opacity_to_alpha\(opacity: u8\) -> u8 \{\s*match opacity \{(.*?)\n\s*\}\s*\}", st, "opacity_to_alpha").group(1)
    table = [int(a) for _, a in re.findall(r"(\d+) => (\d+),", body)]
    rest = int(one(r"_ => (\d+),", body, "opacity_to_alpha's default").group(1))
    out["opacity_to_alpha"] = table + [rest]
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
