"""What temporal accumulation costs and what it buys on C3, one GPU, one
process.

Default: C3 at 1920x1080, 8 bounces, an orbit of `render_view(4)` calls (the
eye stepping along x towards a fixed target), `--calls` timed after `--warmup`:
medians of the accumulate's kernel, of the history's variance kernel and the
iterations of pt_denoise_history, and, in the same loop, of pt_denoise_guided's
iterations on the view itself and of a 4-spp and a 1-spp dispatch.  The
accumulate's floor is its unique traffic -- 64 B of the current view, 68 B of
history, 36 B written per pixel -- at the coalesced 16 B read rate
pt_traffic_probe reports in the same run.  One JSON line.

    python scripts/temporal_bench.py [--width 1920] [--height 1080] [--calls 9] [--warmup 3]

--grid: the defaults' grid instead -- C3 at 96x54, 8 bounces, eight views of 4
spp, the eye stepping 0.05 along x towards the target (the orbit of
tests/test_gpu_temporal.py), against `--clean` frames of the final view from
frame 5000: RMS over RGB of the history and of pt_denoise_history over
max_history x depth_tolerance x normal_cos x albedo_tolerance, beside the raw
final view and pt_denoise_guided of it; then the same orbit at other eye steps
under the defaults.  One JSON line per setting.
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
from compute_path_tracer_amd.path_tracer import PathTracer, look_at_camera  # noqa: E402
from compute_path_tracer_amd.sdf_editor import CompData  # noqa: E402

EYE, TARGET = (2.0, 1.5, -2.5), (0.0, 0.0, 0.0)


def tracer(w, h, bounces):
    prog = scenes.SCENES["c3"]().compile(CompData())
    pt = PathTracer(w, h, prog, settings=N.Settings(debug=0, bounces=bounces, scale=1.0, fov=1.0, aabb=0))
    pt.set_option("jit_wait", 1)  # the values-baked scene kernel, as bench.py's setup
    return pt


def eye_at(k, views, step):
    """View k of `views`: the last one is at EYE, the earlier ones `step` apart along x before it."""
    return (EYE[0] - step * (views - 1 - k), EYE[1], EYE[2])


def cost(args):
    w, h = args.width, args.height
    pt = tracer(w, h, args.bounces)
    total = args.warmup + args.calls
    t = {k: [] for k in ("temporal_ms", "history_variance_ms", "history_denoise_ms", "guided_ms", "variance_ms",
                         "dispatch_4spp_ms", "dispatch_1spp_ms", "guide_ms")}
    for k in range(total):
        pt.render_view(4, look_at_camera(eye_at(k, total, args.step), TARGET))
        row = {"dispatch_4spp_ms": pt.last_dispatch_ms(), "temporal_ms": pt.get_option("temporal_ms"),
               "guide_ms": pt.get_option("guide_ms")}
        pt.denoise_history(iterations=args.iterations)
        row["history_variance_ms"] = pt.get_option("history_variance_ms")
        row["history_denoise_ms"] = pt.get_option("history_denoise_ms")
        pt.denoise_guided(iterations=args.iterations)
        row["guided_ms"], row["variance_ms"] = pt.get_option("guided_ms"), pt.get_option("variance_ms")
        pt.render(1)  # (one more frame of the view; the next render_view clears)
        row["dispatch_1spp_ms"] = pt.last_dispatch_ms()
        if k >= args.warmup:
            for name, v in row.items():
                t[name].append(v)
    count = pt.read_history()[2]
    pt.close()

    ms = (ctypes.c_float * 4)()
    nb = (ctypes.c_uint64 * 4)()
    N.check("pt_traffic_probe", N.lib().pt_traffic_probe(0, 26, ms, nb))
    stream_gbs = nb[1] / (ms[1] * 1e-3) / 1e9  # the coalesced 16 B read
    floor_ms = w * h * (64 + 68 + 36) / (stream_gbs * 1e9) * 1e3
    out = {"width": w, "height": h, "views": total, "eye_step": args.step, "iterations": args.iterations}
    for name, v in t.items():
        out[name] = round(statistics.median(v), 4)
        out[name + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    out.update({"stream16_gbs": round(stream_gbs, 1), "temporal_floor_ms": round(floor_ms, 4),
                "temporal_over_floor": round(out["temporal_ms"] / floor_ms, 2),
                "history_samples_mean": round(float(count.mean()), 2), "history_samples_max": round(float(count.max()), 2)})
    print(json.dumps(out), flush=True)


def grid(args):
    w, h, spp, views = 96, 54, 4, 8
    pt = tracer(w, h, args.bounces)
    pt.set_option("moments", 1)
    aspect = float(np.float32(w) / np.float32(h))
    pt._set_camera(look_at_camera(EYE, TARGET))
    pt.clear()
    pt.dispatch(N.Constants(time=0.0, frame=5000, aspect=aspect, last_clear=0), args.clean)
    clean = pt.read_image()[..., :3].astype(np.float64)

    def rms(img):
        return round(float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - clean) ** 2))), 4)

    def orbit(step, **params):
        pt.reset_history()
        pt.constants.frame = 0
        for k in range(views):
            pt.render_view(spp, look_at_camera(eye_at(k, views, step), TARGET), **params)
        hist, _moments, count = pt.read_history()
        return {"eye_step": step, **params, "raw": rms(pt.read_image()), "history": rms(hist),
                "denoise_guided": rms(pt.denoise_guided()), "denoise_history": rms(pt.denoise_history()),
                "finite": bool(np.isfinite(hist).all()), "samples_mean": round(float(count.mean()), 2),
                "samples_max": round(float(count.max()), 2)}

    for cap in (0.0, 8.0, 16.0, 32.0, 64.0, 1024.0):
        print(json.dumps(orbit(0.05, max_history=cap)), flush=True)
    for name, values in (("depth_tolerance", (0.01, 0.02, 0.1, 0.2)), ("normal_cos", (0.5, 0.8, 0.95, 0.99)),
                         ("albedo_tolerance", (0.02, 0.05, 0.2, 0.5))):
        for v in values:
            print(json.dumps(orbit(0.05, **{name: v})), flush=True)
    for step in (0.0, 0.01, 0.02, 0.1, 0.2, 0.4):
        print(json.dumps(orbit(step)), flush=True)
    for step in (0.0, 0.2):  # the cap at rest, and against the lag of what a mirror shows at a fast orbit
        for cap in (8.0, 16.0, 1024.0):
            print(json.dumps(orbit(step, max_history=cap)), flush=True)
    pt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", type=float, default=0.05)
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--clean", type=int, default=1024)
    args = ap.parse_args()
    (grid if args.grid else cost)(args)


if __name__ == "__main__":
    main()
