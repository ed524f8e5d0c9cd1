"""What a radiance query costs against the simple kernel's dispatch (DESIGN.md
3.32): C3, one GPU, one process.

    python scripts/radiance_bench.py [--runs 3] [--warmup 1] [--width 1920] [--height 1080] [--spp 16] [--bounces 8]

Every pixel's jitter-free primary ray, made on the host from pick_pixels'
geometry and ordered tile by tile as rays_bench.py orders them.  Four device
times, each the median of `--runs` calls after `--warmup`, taken in turn within
every round so that they share the box's state:

  ray_ms         pt_trace_radiance, PT_RADIANCE_RAY, `--spp` samples per ray
                 (radiance_ms; ray_first_ms: its shared first segments)
  hemisphere_ms  pt_trace_radiance, PT_RADIANCE_HEMISPHERE, from the pixels'
                 first-hit points (+ 0.03 normal) about their normals; a pixel
                 that hits nothing gives a NaN ray, which is not traced
                 (hit_share says how many are)
  rays_ms        pt_trace_rays of the same primary rays: the first segment
                 alone, the floor of the shared part
  dispatch_ms    pt_dispatch of `--spp` frames with kernel = 1, the simple
                 kernel: the same interpreter and the same number of paths,
                 with jittered rays and the image fold -- the yardstick

The bar: ray_ms <= dispatch_ms * (1 + dispatch_spread), the spread being the
relative range (max - min) / median of the dispatch's own repeats.  One JSON
line.  PT_LIB picks an A/B build of the library (build.build_variant), e.g.
the ray-fastest layout -DPT_RADIANCE_RAY_FASTEST=1.
"""
import argparse
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
from rays_bench import tile_order  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--scene", default="c3")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    w, h = args.width, args.height
    n = w * h
    prog = scenes.SCENES[args.scene]().compile(CompData())
    pt = PathTracer(w, h, prog, settings=N.Settings(debug=0, bounces=args.bounces, scale=1.0, fov=1.0, aabb=0),
                    options={"kernel": "simple"})
    k = pt._constants(0)
    order = tile_order(w, h)
    xy = np.stack([np.arange(n) % w, np.arange(n) // w], -1).astype(np.int32)[order]
    ro, rd = (np.ascontiguousarray(a) for a in pt._pixel_rays(xy, k))
    hits = pt.pick_pixels(xy, k)
    surface = hits.hit & (hits.shape >= 0)
    with np.errstate(all="ignore"):
        po = np.ascontiguousarray(hits.point + hits.normal * np.float32(0.03))
    po[~surface] = np.nan
    pn = np.ascontiguousarray(hits.normal)

    def radiance(mode):
        o, d = (ro, rd) if mode == "ray" else (po, pn)
        r = pt.trace_radiance(o, d, args.spp, args.bounces, args.seed, mode)
        return r, pt.get_option("radiance_ms"), pt.get_option("radiance_first_ms")

    def rays():
        pt.trace_rays(ro, rd)
        return pt.get_option("rays_ms")

    def dispatch():
        pt.clear()
        pt.dispatch(N.Constants(time=0.0, frame=1, aspect=k.aspect, last_clear=0), args.spp)
        pt.sync()
        return pt.last_dispatch_ms()

    ms = {"ray": [], "ray_first": [], "hemisphere": [], "rays": [], "dispatch": []}
    for r in range(args.warmup + args.runs):
        ray, ray_ms, first_ms = radiance("ray")
        hemi, hemi_ms, hemi_first = radiance("hemisphere")
        assert hemi_first == 0.0
        got = {"ray": ray_ms, "ray_first": first_ms, "hemisphere": hemi_ms, "rays": rays(), "dispatch": dispatch()}
        if r >= args.warmup:
            for name, v in got.items():
                ms[name].append(v)
    image = pt.read_image()[..., :3].reshape(-1, 3)[order]
    line = {"scene": args.scene, "width": w, "height": h, "rays": n, "spp": args.spp, "bounces": args.bounces,
            "runs": args.runs, "warmup": args.warmup, "lib": os.environ.get("PT_LIB", "default"),
            "hit_share": round(float(surface.mean()), 4), "radiance_bytes": int(pt.get_option("radiance_bytes"))}
    pt.close()
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name, v in ms.items():
        line[f"{name}_ms"] = round(med[name], 3)
        line[f"{name}_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
    spread = (max(ms["dispatch"]) - min(ms["dispatch"])) / med["dispatch"]
    line["dispatch_spread"] = round(spread, 4)
    line["ray_over_dispatch"] = round(med["ray"] / med["dispatch"], 4)
    line["hemisphere_over_dispatch"] = round(med["hemisphere"] / med["dispatch"], 4)
    line["ray_clears_the_bar"] = bool(med["ray"] <= med["dispatch"] * (1.0 + spread))
    line["mpaths_per_s_ray"] = round(n * args.spp / med["ray"] / 1e3, 1)
    # the two renders show one picture: the jitter-free query against the jittered image, by their means
    line["mean_radiance_ray"] = [round(float(v), 5) for v in np.nanmean(ray.mean, 0)]
    line["mean_radiance_image"] = [round(float(v), 5) for v in np.nanmean(image, 0)]
    line["mean_irradiance_over_pi"] = [round(float(v), 5) for v in np.nanmean(hemi.mean, 0)]
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
