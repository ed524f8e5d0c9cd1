"""C3 throughput without a sky, with a gradient and with gradient + sun
(pt_set_sky), one GPU: bench.py's timed step (one dispatch of `spp` frames
per step, frames and last_clear running on, one sync at the end) on a
PathTracer whose sky was set first.  One JSON line per sky, with the last
dispatch's trace, shade and sky pass device times.

    python scripts/sky_bench.py [--steps 10] [--warmup 3] [--spp 256]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from compute_path_tracer_amd import _native as N  # noqa: E402
from compute_path_tracer_amd import scenes  # noqa: E402
from compute_path_tracer_amd.distributed import TileSplitRender  # noqa: E402
from compute_path_tracer_amd.path_tracer import PathTracer  # noqa: E402
from compute_path_tracer_amd.sdf_editor import CompData  # noqa: E402

GRADIENT = dict(bottom=(0.9, 0.8, 0.7), top=(0.25, 0.45, 0.9))
SKIES = {"off": None, "gradient": GRADIENT,
         "sun": dict(GRADIENT, sun_direction=(0.4, 0.7, -0.6), sun_color=(8.0, 7.0, 5.0), sun_angle=30.0)}


def run(name, sky, args):
    w, h = args.width, args.height
    prog = scenes.SCENES["c3"]().compile(CompData())
    pt = PathTracer(w, h, prog, settings=N.Settings(debug=0, bounces=args.bounces, scale=1.0, fov=1.0, aabb=0))
    pt.set_option("jit_wait", 1)  # the values-baked scene kernel, as bench.py's setup
    if sky is not None:
        pt.set_sky(**sky)
    tr = TileSplitRender(pt, 0, 1, float(np.float32(w) / np.float32(h)), reduce="host", scaling="strong")
    for _ in range(args.warmup):
        tr.step(args.spp)
    pt.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        tr.step(args.spp)
    pt.sync()
    dt = time.perf_counter() - t0
    img = pt.read_image()
    out = {"sky": name, "msamples_per_s": round(w * h * args.spp * args.steps / dt / 1e6, 1),
           "ms_per_step": round(dt * 1e3 / args.steps, 3), "width": w, "height": h, "spp": args.spp,
           "bounces": args.bounces, "steps": args.steps, "gen_trace": bool(pt.get_option("gen_trace")),
           "gen_norec": bool(pt.get_option("gen_norec")), "trace_ms": round(pt.get_option("trace_ms"), 3),
           "shade_ms": round(pt.get_option("shade_ms"), 3), "sky_ms": round(pt.get_option("sky_ms"), 3),
           "sky_launches": int(pt.get_option("sky_launches")), "mean_rgb": float(np.nanmean(img[..., :3]))}
    pt.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--skies", default="off,gradient,sun")
    args = ap.parse_args()
    for name in args.skies.split(","):
        run(name, SKIES[name], args)


if __name__ == "__main__":
    main()
