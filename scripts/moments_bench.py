"""What the second moments, the variance and the variance-guided filter cost
on C3, one GPU, one process.

Default: bench.py's timed step (one dispatch of `spp` frames per step, frames
and last_clear running on, one sync at the end) with option `moments` off and
on, alternating, `--pairs` times on one context; then, on the image that is
left, the variance kernel and `--iterations` iterations of pt_denoise_guided
against pt_denoise, direct and LDS-staged forms alternating.  One JSON line
per leg and one for the filters.

    python scripts/moments_bench.py [--pairs 3] [--steps 5] [--warmup 1] [--spp 256]

--grid: the default's grid instead -- C3 with the tests' sky at 480x270,
frames 1..n for n in {4, 16, 64} against `--clean` frames from frame 5000, RMS
over RGB of the raw image, pt_denoise's defaults and pt_denoise_guided over
sigma_variance {0.5, 1, 2, 4} x iterations {4, 5}.  One JSON line per n.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from compute_path_tracer_amd import _native as N  # noqa: E402
from compute_path_tracer_amd import scenes  # noqa: E402
from compute_path_tracer_amd.path_tracer import PathTracer  # noqa: E402
from compute_path_tracer_amd.sdf_editor import CompData  # noqa: E402

SKY = dict(bottom=(0.9, 0.8, 0.7), top=(0.25, 0.45, 0.9), sun_direction=(0.4, 0.7, -0.6), sun_color=(8.0, 7.0, 5.0),
           sun_angle=30.0)


def tracer(w, h, bounces):
    prog = scenes.SCENES["c3"]().compile(CompData())
    pt = PathTracer(w, h, prog, settings=N.Settings(debug=0, bounces=bounces, scale=1.0, fov=1.0, aabb=0))
    pt.set_option("jit_wait", 1)  # the values-baked scene kernel, as bench.py's setup
    return pt


def cost(args):
    w, h = args.width, args.height
    aspect = float(np.float32(w) / np.float32(h))
    pt = tracer(w, h, args.bounces)

    def leg(moments):
        pt.set_option("moments", moments)
        pt.clear()
        frame = 0  # (last_clear from 0: with the option on the moments are valid afterwards)

        def step():
            nonlocal frame
            pt.dispatch(N.Constants(time=0.0, frame=1 + frame, aspect=aspect, last_clear=frame), args.spp)
            frame += args.spp

        for _ in range(args.warmup):
            step()
        pt.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        pt.sync()
        dt = time.perf_counter() - t0
        return {"moments": moments, "ms_per_step": round(dt * 1e3 / args.steps, 3),
                "msamples_per_s": round(w * h * args.spp * args.steps / dt / 1e6, 1),
                "last_dispatch_ms": round(pt.last_dispatch_ms(), 3), "trace_ms": round(pt.get_option("trace_ms"), 3),
                "shade_ms": round(pt.get_option("shade_ms"), 3), "bin_chunks": int(pt.get_option("bin_chunks")),
                "moment_frames": int(pt.get_option("moment_frames"))}

    legs = {0: [], 1: []}
    for pair in range(args.pairs):
        for moments in (0, 1):
            out = leg(moments)
            legs[moments].append(out["ms_per_step"])
            print(json.dumps(dict(out, pair=pair, width=w, height=h, spp=args.spp, steps=args.steps)), flush=True)
    off, on = statistics.median(legs[0]), statistics.median(legs[1])
    # the last leg left moments on and valid: the filters run on its image
    pt.render_guides()
    var, fixed, guided, outs = [], {0: [], 1: []}, {0: [], 1: []}, {}
    for k in range(args.filter_warmup + args.calls):
        pt.variance()
        for lds in (0, 1):  # alternating, one box
            pt.set_option("denoise_lds", lds)
            pt.denoise(iterations=args.iterations)
            outs[lds] = pt.denoise_guided(iterations=args.iterations)
            if k >= args.filter_warmup:
                fixed[lds].append(pt.get_option("denoise_ms"))
                guided[lds].append(pt.get_option("guided_ms"))
        if k >= args.filter_warmup:
            var.append(pt.get_option("variance_ms"))
    noise = pt.noise()
    pt.close()

    def med(v):
        return round(statistics.median(v), 4)

    print(json.dumps({
        "moments_off_ms_per_step": off, "moments_on_ms_per_step": on, "on_over_off": round(on / off, 4),
        "off_legs": legs[0], "on_legs": legs[1], "iterations": args.iterations, "variance_ms": med(var),
        "variance_ms_min_max": [round(min(var), 4), round(max(var), 4)],
        "denoise_ms_direct": med(fixed[0]), "denoise_ms_lds": med(fixed[1]), "guided_ms_direct": med(guided[0]),
        "guided_ms_lds": med(guided[1]), "guided_ms_lds_min_max": [round(min(guided[1]), 4), round(max(guided[1]), 4)],
        "guided_forms_bit_identical": bool(np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))),
        "noise_p95": round(noise, 4)}), flush=True)


def grid(args):
    w, h = 480, 270
    aspect = float(np.float32(w) / np.float32(h))
    pt = tracer(w, h, args.bounces)
    pt.set_sky(**SKY)
    pt.set_option("moments", 1)
    pt.render_guides()
    rows, done = [], 0
    for n in (4, 16, 64):
        pt.dispatch(N.Constants(time=0.0, frame=1 + done, aspect=aspect, last_clear=done), n - done)
        done = n
        out = {"raw": pt.read_image(), "pt_denoise": pt.denoise()}
        for it in (4, 5):
            out[f"pt_denoise_{it}"] = pt.denoise(iterations=it)
            for sv in (0.5, 1.0, 2.0, 4.0):
                out[f"guided_{sv}_{it}"] = pt.denoise_guided(iterations=it, sigma_variance=sv)
        rows.append((n, out, pt.noise()))
    pt.clear()
    pt.dispatch(N.Constants(time=0.0, frame=5000, aspect=aspect, last_clear=0), args.clean)
    clean = pt.read_image()[..., :3].astype(np.float64)
    pt.close()
    for n, out, noise in rows:
        ok = np.isfinite(clean).all(-1)
        for img in out.values():
            ok &= np.isfinite(img[..., :3]).all(-1)
        scores = {k: round(float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - clean)[ok] ** 2))), 4)
                  for k, img in out.items()}
        print(json.dumps({"spp": n, "width": w, "height": h, "clean_spp": args.clean, "finite": round(float(ok.mean()), 4),
                          "noise_p95": round(noise, 4), "rms": scores}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--filter-warmup", type=int, default=3)
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--clean", type=int, default=4096)
    args = ap.parse_args()
    (grid if args.grid else cost)(args)


if __name__ == "__main__":
    main()
