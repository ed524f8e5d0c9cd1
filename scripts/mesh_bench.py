"""The mesh extractor's cost on C3, one GPU, one process: pt_mesh_extract of a
box that holds the scene at 128^3, 256^3 and 512^3 (the longest axis), with
the brick skip on and off alternating, each point repeated until it holds at
least half a second of device time (HIP events around every stage's kernels).
Per point: ms per stage, corner evaluations per second of the classify stage,
the share of bricks evaluated, vertices and triangles, and whether the two
forms gave the same bytes.  Beside it, as a yardstick and not a bar: the march
kernel's map() rate from a stats run of the same scene (march steps over the
binned trace passes' device time), for the scene kernel and the interpreter.
One JSON line per point, then one for the yardstick.

    python scripts/mesh_bench.py [--resolutions 128 256 512] [--seconds 0.5] [--warmup 2] [--project 2]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from compute_path_tracer_amd import _native as N  # noqa: E402
from compute_path_tracer_amd import scenes  # noqa: E402
from compute_path_tracer_amd.path_tracer import PathTracer, mesh_grid  # noqa: E402
from compute_path_tracer_amd.sdf_editor import CompData  # noqa: E402

# C3's room: floor and roof reach |x| 11.63 and |z| 12.26, the tilted back wall z 13.3, y from -3.32 to 4.25
BOX_MIN, BOX_MAX = (-12.5, -4.0, -13.0), (12.5, 5.0, 14.0)
STAGES = ("skip", "classify", "scan", "emit")


def extract(pt, desc):
    """One pt_mesh_extract without the readback: (info, ms per stage)."""
    info = N.MeshInfo()
    N.check("pt_mesh_extract", pt._L.pt_mesh_extract(pt._ctx, ctypes.byref(desc), ctypes.byref(info)), pt._ctx)
    return info, {s: pt.get_option(f"mesh_{s}_ms") for s in STAGES}


def digest(mesh):
    h = hashlib.sha256()
    for a in (mesh.positions, mesh.normals, mesh.shapes, mesh.triangles):
        h.update(a.tobytes())
    return h.hexdigest()


def march_rate(prog, jit, width=1920, height=1080, spp=4, bounces=8):
    pt = PathTracer(width, height, prog, settings=N.Settings(debug=0, bounces=bounces, scale=1.0, fov=1.0, aabb=0),
                    options={"kernel": "binned", "jit": jit})
    if jit:
        pt.set_option("jit_wait", 1)
    k = N.Constants(time=0.0, frame=1, aspect=float(np.float32(width) / np.float32(height)), last_clear=1)
    ms = []
    for _ in range(4):
        pt.clear()
        pt.dispatch(k, spp)
        pt.sync()
        ms.append(pt.get_option("trace_ms"))
    steps = pt.stats(k, spp)["march_steps"]
    pt.close()
    trace_ms = statistics.median(ms[1:])
    return {"march_steps": steps, "trace_ms": round(trace_ms, 3), "maps_per_s": round(steps / (trace_ms * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--project", type=int, default=2)
    args = ap.parse_args()
    prog = scenes.SCENES["c3"]().compile(CompData())
    pt = PathTracer(16, 16, prog, settings=N.Settings(debug=0, bounces=2, scale=1.0, fov=1.0, aabb=0), options={"jit": 0})
    for res in args.resolutions:
        origin, cell, cells = mesh_grid(BOX_MIN, BOX_MAX, res)
        desc = N.MeshDesc(cell=float(cell), iso=0.0, project=args.project)
        for k in range(3):
            desc.origin[k], desc.cells[k] = float(origin[k]), cells[k]
        runs = {1: [], 0: []}
        infos, hashes = {}, {}
        for skip in (1, 0):  # the bytes of both forms, once
            pt.set_option("mesh_skip", skip)
            hashes[skip] = digest(pt.extract_mesh(grid=(origin, cell, cells), project=args.project))
        k = 0
        while k < args.warmup or min(sum(sum(r.values()) for r in runs[s]) for s in (0, 1)) < args.seconds * 1e3:
            for skip in (1, 0):  # alternating, one process
                pt.set_option("mesh_skip", skip)
                infos[skip], ms = extract(pt, desc)
                if k >= args.warmup:
                    runs[skip].append(ms)
            k += 1
        for skip in (1, 0):
            info = infos[skip]
            med = {s: statistics.median(r[s] for r in runs[skip]) for s in STAGES}
            totals = [sum(r.values()) for r in runs[skip]]
            print(json.dumps({
                "resolution": res, "cells": list(cells), "cell": float(cell), "mesh_skip": skip, "project": args.project,
                "runs": len(totals), "ms": {s: round(v, 3) for s, v in med.items()},
                "mesh_ms": round(statistics.median(totals), 3), "mesh_ms_min_max": [round(min(totals), 3), round(max(totals), 3)],
                "corner_evals": int(info.corner_evals),
                "corner_evals_per_s_classify": round(info.corner_evals / (med["classify"] * 1e-3)) if med["classify"] else None,
                "bricks": int(info.bricks), "bricks_evaluated": int(info.bricks_evaluated),
                "evaluated_share": round(info.bricks_evaluated / info.bricks, 4),
                "vertices": int(info.n_vertices), "triangles": int(info.n_triangles),
                "clipped_edges": int(info.clipped_edges), "device_mib": round(info.device_bytes / 2 ** 20, 1),
                "forms_bit_identical": hashes[0] == hashes[1]}), flush=True)
    pt.close()
    print(json.dumps({"yardstick": "march kernel map() rate, C3 1920x1080 4 spp 8 bounces, binned trace passes",
                      "scene_kernel": march_rate(prog, 1), "interpreter": march_rate(prog, 0)}), flush=True)


if __name__ == "__main__":
    main()
