"""The denoiser's cost on C3, one GPU, one process: the guide images, the
a-trous filter (direct and LDS-staged form, alternating calls), the 1-spp and
4-spp dispatches of the same context (the preview the filter competes with),
and the coalesced 16 B read rate of pt_traffic_probe, from which the filter's
floor follows: iterations x W*H x 64 B (16 B colour + 32 B guides read, 16 B
written) at that rate.  One JSON line.

    python scripts/denoise_bench.py [--width 1920] [--height 1080] [--calls 9] [--warmup 3] [--save DIR]

--save DIR writes DIR/denoise_in.png and DIR/denoise_out.png: the 4-spp image
with a sky and its denoised form (save_png), for looking at the defaults.
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
from compute_path_tracer_amd.path_tracer import PathTracer, save_png  # noqa: E402
from compute_path_tracer_amd.sdf_editor import CompData  # noqa: E402

SKY = dict(bottom=(0.9, 0.8, 0.7), top=(0.25, 0.45, 0.9), sun_direction=(0.4, 0.7, -0.6), sun_color=(8.0, 7.0, 5.0),
           sun_angle=30.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--save", default=None)
    args = ap.parse_args()
    w, h = args.width, args.height
    prog = scenes.SCENES["c3"]().compile(CompData())
    pt = PathTracer(w, h, prog, settings=N.Settings(debug=0, bounces=args.bounces, scale=1.0, fov=1.0, aabb=0))
    pt.set_option("jit_wait", 1)  # the values-baked scene kernel, as bench.py's setup
    pt.set_sky(**SKY)
    aspect = float(np.float32(w) / np.float32(h))

    def dispatch_ms(spp):
        times = []
        for k in range(args.warmup + args.calls):
            pt.clear()
            pt.dispatch(N.Constants(time=0.0, frame=1, aspect=aspect, last_clear=1), spp)
            if k >= args.warmup:
                times.append(pt.last_dispatch_ms())
        return statistics.median(times)

    spp1_ms = dispatch_ms(1)
    spp4_ms = dispatch_ms(4)  # (leaves the 4-spp image the filter runs on)
    guide = []
    for k in range(args.warmup + args.calls):
        pt.render_guides()
        if k >= args.warmup:
            guide.append(pt.get_option("guide_ms"))
    den = {0: [], 1: []}
    outs = {}
    for k in range(args.warmup + args.calls):
        for lds in (0, 1):  # alternating, one box
            pt.set_option("denoise_lds", lds)
            outs[lds] = pt.denoise(iterations=args.iterations)
            if k >= args.warmup:
                den[lds].append(pt.get_option("denoise_ms"))
    same = bool(np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)))
    if args.save:
        os.makedirs(args.save, exist_ok=True)
        save_png(pt.read_image(), os.path.join(args.save, "denoise_in.png"))
        save_png(outs[0], os.path.join(args.save, "denoise_out.png"))
    pt.close()

    ms = (ctypes.c_float * 4)()
    nb = (ctypes.c_uint64 * 4)()
    N.check("pt_traffic_probe", N.lib().pt_traffic_probe(0, 26, ms, nb))
    stream_gbs = nb[1] / (ms[1] * 1e-3) / 1e9  # the coalesced 16 B read
    floor_ms = args.iterations * w * h * 64 / (stream_gbs * 1e9) * 1e3
    direct, lds = statistics.median(den[0]), statistics.median(den[1])
    print(json.dumps({
        "width": w, "height": h, "iterations": args.iterations, "guide_ms": round(statistics.median(guide), 3),
        "denoise_ms_direct": round(direct, 3), "denoise_ms_lds": round(lds, 3),
        "denoise_ms_direct_min_max": [round(min(den[0]), 3), round(max(den[0]), 3)],
        "denoise_ms_lds_min_max": [round(min(den[1]), 3), round(max(den[1]), 3)], "forms_bit_identical": same,
        "dispatch_1spp_ms": round(spp1_ms, 3), "dispatch_4spp_ms": round(spp4_ms, 3),
        "stream16_gbs": round(stream_gbs, 1), "floor_ms": round(floor_ms, 3),
        "direct_over_floor": round(direct / floor_ms, 2), "lds_over_floor": round(lds / floor_ms, 2)}), flush=True)


if __name__ == "__main__":
    main()
