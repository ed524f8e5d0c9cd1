"""What a ray query costs against the guide kernel: C3, one
GPU, one process.

    python scripts/rays_bench.py [--runs 10] [--warmup 3] [--width 1920] [--height 1080]

Four kernel times, each the median of `--runs` calls after `--warmup`, the
four taken in turn within every round so that they share the box's state:

  guide_ms      pt_render_guides: the same march and normals for the same
                rays, one wave per 8x8 tile -- the yardstick
  pick_ms       pt_pick_pixels over every pixel (the NULL list)
  rays_ms       pt_trace_rays over those same primary rays, made on the host
                from the guides' camera, in the guide kernel's order (tile by
                tile, so a wave marches the rays the guide kernel's wave does);
                rays_rows_ms: the same rays in image order (a wave = 64 pixels
                of one row)
  shuffled_ms   pt_trace_rays over a random permutation of them: the
                incoherent case

and that the three forms give one answer: (normal, t) of the pick and of the
caller rays equal the guide plane g0 bit for bit.  One JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from compute_path_tracer_amd import _native as N  # noqa: E402
from compute_path_tracer_amd import scenes  # noqa: E402
from compute_path_tracer_amd.path_tracer import PathTracer  # noqa: E402
from compute_path_tracer_amd.sdf_editor import CompData  # noqa: E402


def tile_order(w, h):
    """Image-order indices of the pixels in the guide kernel's order: 8x8 tiles row by row, 8 rows of 8 in each."""
    assert w % 8 == 0 and h % 8 == 0, "whole tiles only: the rays then are exactly the guide kernel's"
    idx = np.arange(w * h, dtype=np.int64).reshape(h // 8, 8, w // 8, 8)
    return idx.transpose(0, 2, 1, 3).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="c3")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    w, h = args.width, args.height
    n = w * h
    prog = scenes.SCENES[args.scene]().compile(CompData())
    pt = PathTracer(w, h, prog, settings=N.Settings(debug=0, bounces=8, scale=1.0, fov=1.0, aabb=0))
    k = pt._constants(0)
    xy = np.stack([np.arange(n) % w, np.arange(n) // w], -1).astype(np.int32)
    ro, rd = pt._pixel_rays(xy, k)  # image order
    order = {"rays": tile_order(w, h), "rays_rows": np.arange(n), "shuffled": np.random.default_rng(args.seed).permutation(n)}
    rays = {name: (np.ascontiguousarray(ro[p]), np.ascontiguousarray(rd[p])) for name, p in order.items()}
    t, shape, nrm = np.empty(n, np.float32), np.empty(n, np.int32), np.empty((n, 3), np.float32)
    out = (N.fptr(t), N.ptr(shape, ctypes.c_int32), N.fptr(nrm))
    L, ctx = pt._L, pt._ctx

    def trace(name):
        o, d = rays[name]
        pt._chk("pt_trace_rays", L.pt_trace_rays(ctx, N.fptr(o), N.fptr(d), n, *out))
        return pt.get_option("rays_ms")

    def pick():
        pt._chk("pt_pick_pixels", L.pt_pick_pixels(ctx, ctypes.byref(k), ctypes.byref(pt.settings), None, n, *out))
        return pt.get_option("pick_ms")

    def guides():
        pt.render_guides(k)
        return pt.get_option("guide_ms")

    ms = {"guide": [], "pick": [], "rays": [], "rays_rows": [], "shuffled": []}
    for r in range(args.warmup + args.runs):
        got = {"guide": guides(), "pick": pick(), "rays": trace("rays"), "rays_rows": trace("rays_rows"),
               "shuffled": trace("shuffled")}
        if r >= args.warmup:
            for name, v in got.items():
                ms[name].append(v)
    # one answer: the pick and the caller rays against the guide plane
    g0, g1 = pt.read_guides()
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    same = lambda a, b: bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())  # noqa: E731
    pick()
    pick_same = same(t.reshape(h, w), g0[..., 3]) and same(nrm.reshape(h, w, 3), g0[..., :3])
    trace("rays_rows")
    rays_same = same(t.reshape(h, w), g0[..., 3]) and same(nrm.reshape(h, w, 3), g0[..., :3])
    hits = float(g1[..., 3].mean())
    pt.close()
    med = {name: statistics.median(v) for name, v in ms.items()}
    line = {"scene": args.scene, "width": w, "height": h, "rays": n, "runs": args.runs, "warmup": args.warmup,
            "hit_share": round(hits, 4)}
    for name, v in ms.items():
        line[f"{name}_ms"] = round(med[name], 4)
        line[f"{name}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    for name in ("pick", "rays", "rays_rows", "shuffled"):
        line[f"{name}_over_guide"] = round(med[name] / med["guide"], 4)
    line["mrays_per_s_coherent"] = round(n / med["rays"] / 1e3, 1)
    line["mrays_per_s_shuffled"] = round(n / med["shuffled"] / 1e3, 1)
    line["pick_equals_guides"] = pick_same
    line["rays_equal_guides"] = rays_same
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
