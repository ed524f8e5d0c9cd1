"""The mesh export's host side: the grid ``PathTracer.extract_mesh`` lays over
a box, and the ``Mesh`` it returns with its OBJ / PLY writers.  No context."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native as N


def mesh_grid(box_min, box_max, resolution: int):
    """The grid ``extract_mesh`` lays over a box, in float32 steps: cubic cells
    of edge cell = max(box_max - box_min) / resolution, so the longest axis
    gets ``resolution`` cells and every other axis ceil(extent / cell) (at
    least 1); origin = box_min.  Returns (origin float32[3], cell float32,
    cells (nx, ny, nz)).  Host arithmetic only (no context)."""
    F = np.float32
    lo, hi = np.asarray(box_min, dtype=F), np.asarray(box_max, dtype=F)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError(f"box corners must be three finite numbers each, got {box_min!r}, {box_max!r}")
    ext = hi - lo
    if not (ext > 0).all():
        raise ValueError(f"box_max must exceed box_min on every axis, got {box_min!r}, {box_max!r}")
    if not 1 <= int(resolution) <= N.PT_MESH_MAX_CELLS:
        raise ValueError(f"resolution must lie in [1, {N.PT_MESH_MAX_CELLS}], got {resolution!r}")
    cell = F(ext.max() / F(int(resolution)))
    cells = tuple(int(min(N.PT_MESH_MAX_CELLS, max(1, np.ceil(e / cell)))) for e in ext)
    return lo, cell, cells


class Mesh:
    """A triangle mesh as ``PathTracer.extract_mesh`` returns it: ``positions``
    and ``normals`` float32 [n][3], ``shapes`` int32 [n] (ordinal of the
    program's SHAPE op whose material map() returns at the vertex, -1 = none),
    ``triangles`` uint32 [m][3] wound outward, ``info`` the extractor's counts
    (a dict of pt_mesh_info's fields)."""

    def __init__(self, positions, normals, shapes, triangles, info=None):
        self.positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self.shapes = np.ascontiguousarray(shapes, np.int32).reshape(-1)
        self.triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        self.info = dict(info or {})

    def vertex_colors(self, program, data: Optional[np.ndarray] = None) -> np.ndarray:
        """Each vertex's albedo, float32 [n][3]: the first three material slots
        of its shape op in ``data`` (default: the values of ``program``, a
        sdf_editor.Program); MDEF's black where no shape claims the vertex."""
        d = np.asarray(program.data if data is None else data, np.float32)
        slots = [list(program.ops[i].material[:3]) for i in range(program.n_ops)
                 if program.ops[i].opcode == N.PT_OP_SHAPE]
        table = np.zeros((len(slots) + 1, 3), np.float32)  # row 0: shape -1
        for k, s in enumerate(slots):
            table[k + 1] = d[s]
        if len(self.shapes) and (self.shapes.min() < -1 or self.shapes.max() >= len(slots)):
            raise ValueError("mesh shape ordinal outside the program's shape ops")
        return table[self.shapes + 1]

    def bake_rays(self, mode: str = "irradiance", offset: float = 0.03):
        """The rays ``PathTracer.bake_mesh`` traces, one per vertex, float32
        [n][3] each, from p + n * offset in float32 steps (0.03: the path's own
        bounce offset): "irradiance" -> (origins, n), the normals a hemisphere
        query draws its directions about; "view" -> (origins, -n), the ray of
        a viewer looking straight at the vertex.  Host arithmetic only."""
        if mode not in ("irradiance", "view"):
            raise ValueError(f'mode must be "irradiance" or "view", got {mode!r}')
        origins = self.positions + self.normals * np.float32(offset)
        return origins, (self.normals.copy() if mode == "irradiance" else -self.normals)

    def lit_colors(self, radiance, program=None, data: Optional[np.ndarray] = None) -> np.ndarray:
        """Display colours from a ``bake_mesh`` result, float32 [n][3] in 0..1,
        ready for ``save_ply(colors=)``: the mean of a "view" bake, or albedo x
        mean (``vertex_colors(program, data)``) of an "irradiance" bake -- the
        light a diffuse surface sends on -- then clip(., 0, 1) ** (1 / 2.2).
        A NaN stays one (``save_ply`` paints it black)."""
        mean = np.asarray(radiance.mean, np.float32)
        if mean.shape != self.positions.shape:
            raise ValueError(f"radiance must hold one row per vertex {self.positions.shape}, got {mean.shape}")
        if radiance.mode == "hemisphere":
            if program is None:
                raise ValueError("an irradiance bake needs the program for the vertices' albedo")
            mean = self.vertex_colors(program, data) * mean
        with np.errstate(all="ignore"):
            return (np.clip(mean, np.float32(0.0), np.float32(1.0)) ** np.float32(1.0 / 2.2)).astype(np.float32)

    def save_obj(self, path: str) -> None:
        """Wavefront OBJ: ``v``, ``vn`` and ``f a//a b//b c//c`` records (1-based)."""
        with open(path, "w") as f:
            f.write("# compute_path_tracer_amd mesh export\n")
            for p in self.positions:
                f.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p))
            for n in self.normals:
                f.write("vn %.9g %.9g %.9g\n" % tuple(float(x) for x in n))
            for t in self.triangles:
                a, b, c = (int(i) + 1 for i in t)
                f.write(f"f {a}//{a} {b}//{b} {c}//{c}\n")

    def save_ply(self, path: str, colors: Optional[np.ndarray] = None) -> None:
        """Binary little-endian PLY: x y z nx ny nz per vertex (+ uchar red
        green blue from ``colors``, float [n][3] in 0..1), a uchar count and
        three int32 indices per face."""
        nv, nt = len(self.positions), len(self.triangles)
        fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header = ["ply", "format binary_little_endian 1.0", "comment compute_path_tracer_amd mesh export",
                  f"element vertex {nv}"] + [f"property float {n}" for n, _ in fields]
        if colors is not None:
            col = np.asarray(colors, np.float32)
            if col.shape != (nv, 3):
                raise ValueError(f"colors must be ({nv}, 3), got {col.shape}")
            fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
            header += ["property uchar red", "property uchar green", "property uchar blue"]
        header += [f"element face {nt}", "property list uchar int vertex_indices", "end_header"]
        v = np.zeros(nv, dtype=np.dtype(fields))
        for k, name in enumerate(("x", "y", "z")):
            v[name] = self.positions[:, k]
            v["n" + name] = self.normals[:, k]
        if colors is not None:
            c8 = np.rint(np.clip(np.nan_to_num(col), 0.0, 1.0) * 255.0).astype(np.uint8)
            v["red"], v["green"], v["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
        fc = np.zeros(nt, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
        fc["n"] = 3
        fc["i"] = self.triangles.astype(np.int32)
        with open(path, "wb") as f:
            f.write(("\n".join(header) + "\n").encode("ascii"))
            f.write(v.tobytes())
            f.write(fc.tobytes())
