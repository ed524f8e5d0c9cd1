"""What the preview shading costs against the guide kernel and against the
path tracer's own small dispatches: C3 under
look_at(EYE, TARGET) with the tests' sky, one GPU, one process.

    python scripts/preview_bench.py [--runs 10] [--warmup 3] [--width 1920] [--height 1080]

Seven device times, each the median of `--runs` calls after `--warmup`, the
seven taken in turn within every round so that they share the box's state:

  preview_off_ms      pt_render_preview, shadow and occlusion off: the guide
                      kernel's work plus the light's few multiplies
  preview_ao_ms       occlusion only (five map() taps at all checks per hit)
  preview_shadow_ms   shadow at all checks, no occlusion (32 steps at most)
  preview_cull_ms     shadow under bounds() of the shadow ray, no occlusion
  preview_full_ms     PathTracer.preview's defaults: shadow at all checks and
                      occlusion
  guide_ms            pt_render_guides: the same first hits -- the yardstick
  spp1_ms, spp4_ms    a 1-spp and a 4-spp dispatch of the path tracer (the
                      automatic kernel choice), from pt_last_dispatch_ms

The light is preview_light's: the sky's sun.  The setting with both terms off
is also checked against the guides (albedo and hit flag where nothing emits).
One JSON line.
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

EYE, TARGET = (2.0, 1.5, -2.5), (0.0, 0.0, 0.0)  # tests/gpuharness.py
SKY = dict(bottom=(0.9, 0.8, 0.7), top=(0.25, 0.45, 0.9), sun_direction=(0.4, 0.7, -0.6), sun_color=(8.0, 7.0, 5.0),
           sun_angle=30.0)
SETTINGS = {"off": dict(shadow_steps=0, ao_strength=0.0), "ao": dict(shadow_steps=0),
            "shadow": dict(ao_strength=0.0), "cull": dict(ao_strength=0.0, shadow_cull=True), "full": {}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="c3")
    args = ap.parse_args()
    w, h = args.width, args.height
    prog = scenes.SCENES[args.scene]().compile(CompData())
    pt = PathTracer(w, h, prog, settings=N.Settings(debug=0, bounces=8, scale=1.0, fov=1.0, aabb=0))
    pt.look_at(EYE, TARGET)
    pt.set_sky(**SKY)
    pt.update()
    pt.set_option("jit_wait", 1)  # the values-baked scene kernel for the dispatches, as bench.py's setup

    def preview(name):
        img = pt.preview(**SETTINGS[name])
        return pt.get_option("preview_ms"), img

    def guides():
        pt.render_guides()
        return pt.get_option("guide_ms")

    def dispatch(spp):
        pt.render(spp)
        pt.sync()
        return pt.last_dispatch_ms()

    ms = {f"preview_{name}": [] for name in SETTINGS}
    ms.update({"guide": [], "spp1": [], "spp4": []})
    for r in range(args.warmup + args.runs):
        got = {f"preview_{name}": preview(name)[0] for name in SETTINGS}
        got.update({"guide": guides(), "spp1": dispatch(1), "spp4": dispatch(4)})
        if r >= args.warmup:
            for name, v in got.items():
                ms[name].append(v)
    # what the images hold: the classes by the shadow term's effect, and the neutral image against the guides
    g0, g1 = pt.read_guides()
    hit = g1[..., 3] != 0
    off, shadow, cull, full = (preview(name)[1] for name in ("off", "shadow", "cull", "full"))
    one = (1.0, 1.0, 1.0)
    neutral = pt.preview(light_color=(0.0, 0.0, 0.0), ambient=(one, one), shadow_steps=0, ao_strength=0.0)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    differs = lambda a, b: (bits(a) != bits(b)).any(-1)  # noqa: E731
    alpha_same = bool(np.array_equal(neutral[..., 3], g1[..., 3]))
    albedo_share = float((~differs(neutral[..., :3], g1[..., :3]))[hit].mean()) if hit.any() else 1.0
    pt.close()
    med = {name: statistics.median(v) for name, v in ms.items()}
    line = {"scene": args.scene, "width": w, "height": h, "runs": args.runs, "warmup": args.warmup,
            "hit_share": round(float(hit.mean()), 4)}
    for name, v in ms.items():
        line[f"{name}_ms"] = round(med[name], 4)
        line[f"{name}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    for name in SETTINGS:
        line[f"preview_{name}_over_guide"] = round(med[f"preview_{name}"] / med["guide"], 4)
    line["preview_full_over_spp1"] = round(med["preview_full"] / med["spp1"], 4)
    line["shadow_changes_share"] = round(float(differs(off, shadow)[hit].mean()), 4) if hit.any() else 0.0
    line["cull_changes_share"] = round(float(differs(shadow, cull)[hit].mean()), 4) if hit.any() else 0.0
    line["finite"] = bool(np.isfinite(full).all())
    line["neutral_alpha_equals_g1"] = alpha_same
    line["neutral_rgb_equals_albedo_share"] = round(albedo_share, 4)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
