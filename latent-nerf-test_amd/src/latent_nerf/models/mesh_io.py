"""Wavefront OBJ output of NeRFRenderer.export_mesh: `v x y z r g b`, `vn` and `f a//a b//b c//c` lines (or, textured,
`v`, `vt`, `vn`, `f a/t/a ...` and a material file), formatted by
one format operation over each whole array (no per-line Python loop).  The file reads back through src/latent_paint/models/mesh.py
read_obj (and any viewer that takes per-vertex colours after the position)."""
import os

import numpy as np


def _fmt_rows(fmt, arr):
    # the row format repeated V times and applied once to the flattened array: no per-line Python loop
    text = (fmt + "\n") * len(arr)
    return text % tuple(arr.reshape(-1).tolist())


def write_obj(path, verts, faces, normals=None, colors=None):
    """verts [V,3], faces [F,3] (0-based), normals [V,3] | None, colors [V,3] in [0,1] | None (numpy or CPU tensors)."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# %d vertices, %d triangles\n" % (len(verts), len(faces)))
        if colors is not None:
            colors = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
            f.write(_fmt_rows("v %.9g %.9g %.9g %.4f %.4f %.4f", np.concatenate([verts, colors], 1)))
        else:
            f.write(_fmt_rows("v %.9g %.9g %.9g", verts))
        if normals is not None:
            f.write(_fmt_rows("vn %.6f %.6f %.6f", np.asarray(normals, dtype=np.float32).reshape(-1, 3)))
            f.write(_fmt_rows("f %d//%d %d//%d %d//%d", np.repeat(faces + 1, 2, axis=1)))
        else:
            f.write(_fmt_rows("f %d %d %d", faces + 1))
    return path


def write_textured_obj(path, verts, faces, vt, ft, normals=None, material="mesh.mtl", texture="albedo.png"):
    """Textured OBJ: `mtllib`, `v`, `vt` (%.9g: f32 survives the round trip), `vn`, `usemtl` and `f v/vt/vn` (or
    `f v/vt` without normals), plus the material file `material` next to it naming `texture` as its map_Kd.
    verts [V,3], faces [F,3], vt [T,2], ft [F,3] (0-based), normals [V,3] | None (numpy or CPU tensors)."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vt = np.asarray(vt, dtype=np.float32).reshape(-1, 2)
    ft = np.asarray(ft, dtype=np.int64).reshape(-1, 3)
    out_dir = os.path.dirname(os.path.abspath(path))
    os.makedirs(out_dir, exist_ok=True)
    with open(path, "w") as f:
        f.write("# %d vertices, %d texture vertices, %d triangles\n" % (len(verts), len(vt), len(faces)))
        f.write("mtllib %s\n" % material)
        f.write(_fmt_rows("v %.9g %.9g %.9g", verts))
        f.write(_fmt_rows("vt %.9g %.9g", vt))
        f.write("usemtl material0\n")
        if normals is not None:
            f.write(_fmt_rows("vn %.6f %.6f %.6f", np.asarray(normals, dtype=np.float32).reshape(-1, 3)))
            corners = np.stack([faces + 1, ft + 1, faces + 1], -1).reshape(-1, 9)
            f.write(_fmt_rows("f %d/%d/%d %d/%d/%d %d/%d/%d", corners))
        else:
            f.write(_fmt_rows("f %d/%d %d/%d %d/%d", np.stack([faces + 1, ft + 1], -1).reshape(-1, 6)))
    with open(os.path.join(out_dir, material), "w") as f:
        f.write("newmtl material0\nKa 1.000000 1.000000 1.000000\nKd 1.000000 1.000000 1.000000\n"
                "Ks 0.000000 0.000000 0.000000\nillum 1\nNs 0.000000\nmap_Kd %s\n" % texture)
    return path
