"""Shared by test_reuse_ref.py (no GPU) and test_gpu_reuse.py: walks of one
long-lived context through reconfiguration, as data, and the oracle's image
after every step.  A step is an absolute description of the context (scene,
window, tiles, bounces, debug, kernel and binned options, moments, sky,
camera) and of what to render (spp, stats() first or not, cleared or
accumulating), so a walk can run in any order; apply() makes only the calls
that take a context from one step to the next.  Also here, from the step data
alone: which of the transitions a to j (TRANSITIONS) a walk contains, and a
model of what the binned pipeline's buffers hold after each step
(pt_bin_host.cpp ensure_bin / plan_dispatch).  No GPU and no library state."""
import dataclasses
import functools
import random
import re
from pathlib import Path
from typing import Optional

import numpy as np

import camref
import gpuharness as G
from compute_path_tracer_amd import _native as N, scenes
from compute_path_tracer_amd.sdf_editor import CompData
from oracle import oracle as O

TILE = 8
# pt_binned.h PT_BIN_BITS (test_reuse_ref.py reads the header): a scene whose check[] set fits the bin
# index, one that goes through the table of sets (up to 64 entries), one with the wide masks
BIN_BITS = 12
# per sample of a lane (test_gpu_options.py), and the wide buffers' share (mask_hi uint2 + hitn float4)
BYTES_PER_SAMPLE = 2 * 64 + 16 + 8 + 16
BYTES_WIDE = 8 + 16
# test_work_counters_match_oracle's keys
COUNTERS = ("samples", "segments", "march_steps", "normal_maps", "shaded", "aabb_tests", "xform_union", "xform_shape",
            "sdf_sphere", "sdf_cube", "sdf_octahedron", "comb_union", "comb_sub", "comb_assign", "rr_break")
SEEDS = (20251, 7919)

INTERP = ("binned",)
SCENEK = ("binned_jit", "binned_jit_trace_taps", "binned_tier")
VARIANTS = {"PIPELINE": ("binned", "binned_jit", "binned_jit_trace_taps", "binned_tier"),
            "GENERIC": ("simple", "wave", "jit")}
TIER_STEPS = 5  # binned_tier runs the last five steps of the scene-kernel walk


@dataclasses.dataclass(frozen=True)
class Step:
    label: str
    # configuration
    scene: str = "c3"
    w: int = 40
    h: int = 24
    tiles: tuple = (0, 1)  # set_tiles(rank, nranks)
    bounces: int = 3
    debug: int = 0
    kernel: Optional[str] = None  # "simple" / "wave" / "auto" / "binned"; None: the variant's own
    lanes: Optional[int] = None  # bin_lanes, bin_samples, bin_table (None: not named, the GENERIC walk)
    samples: Optional[int] = None
    table: Optional[int] = None
    moments: int = 0
    sky: bool = False  # G.SKY
    camera: str = "default"  # a G.LOOK name
    # what to render
    spp: int = 2
    stats: bool = False  # stats() before the dispatch
    clear: bool = True  # False: accumulation goes on from the step before (same group)
    group: Optional[str] = None  # steps of one group move as one unit
    only: Optional[tuple] = None  # the variants that run it (None: all of the walk's)
    variant: Optional[str] = None  # filled in by walk()


def render_key(s):
    """What determines a cleared step's image."""
    return (s.scene, s.w, s.h, s.tiles, s.bounces, s.debug, s.spp, s.sky, s.camera)


# -- the walks ---------------------------------------------------------------
def _pipeline():
    P = functools.partial(Step, lanes=2, samples=1 << 20, table=1)
    acc = functools.partial(P, bounces=4, group="acc")
    mom = functools.partial(P, bounces=5, group="mom", only=INTERP)
    return [
        P("a: 72x40, 5 spp: the largest capacity", w=72, h=40, spp=5),
        P("a: down to 24x16", w=24, h=16),
        P("a: up to 64x48", w=64, h=48),
        P("a: ragged 9x17: gen, scan, scatter first pass", w=9, h=17, spp=3),
        P("a: whole tiles again, 40x24"),
        P("b: 8 bounces", bounces=8),
        P("b: 0 bounces: one pass", bounces=0),
        P("b: 32 bounces: ctrl grows", bounces=32),
        P("b: 3 bounces", spp=3),
        P("c: 1 lane", w=32, h=16, lanes=1, spp=3),
        P("c: 4 lanes, 2 frames", w=32, h=16, lanes=4, spp=2),
        P("c: 2 lanes", w=32, h=16, lanes=2, spp=4),
        P("c: 3 lanes", w=32, h=16, lanes=3, spp=5),
        P("d: bin_samples 64: a chunk per frame", w=24, h=16, samples=64, spp=3),
        P("d: bin_samples 1 << 20: one chunk", w=24, h=16, spp=4),
        P("g: debug 1", bounces=8, debug=1),
        P("g: debug 3", bounces=8, debug=3),
        P("g: debug 0 again", bounces=8, spp=3),
        P("j: lens and sky on c2", scene="c2", w=12, h=8, spp=1, sky=True, camera="lens"),
        P("j: lens and sky on c3", w=12, h=8, spp=1, sky=True, camera="lens"),
        P("j: default camera, no sky", w=12, h=8),
        acc("i: 2 spp, 1 lane", lanes=1),
        acc("i: + 3 spp, 3 lanes, bin_samples 64", lanes=3, samples=64, spp=3, clear=False),
        acc("i: + 2 spp on simple", lanes=3, samples=64, kernel="simple", clear=False),
        acc("i: + 2 spp on wave", lanes=3, samples=64, kernel="wave", clear=False),
        acc("i: + 2 spp on auto", lanes=3, samples=64, kernel="auto", clear=False),
        mom("i: 2 spp, moments 0"),
        mom("i: + 3 spp, moments 1", moments=1, spp=3, clear=False),
        mom("i: + 2 spp, moments 0", clear=False),
        P("e: cull, 64 entries", scene="cull", w=48, only=INTERP),
        P("e: c3 with bin_table 0", w=48, table=0, spp=4),
        P("e: c2, the set is the bin index", scene="c2", w=48),
        P("e: c3, the table of sets", w=48),
        P("e: wide, hash bins and the wide masks", scene="wide", w=48, only=INTERP),
        P("e: c3_noaabb, every mask empty", scene="c3_noaabb", w=48, spp=5, only=INTERP),
        P("e: c1, one entry", scene="c1", w=48, only=SCENEK),
        P("e: back to c3", w=48, spp=3),
        P("e: back to c2", scene="c2", w=48, spp=3),
        P("f: stats() first on c3", w=24, h=16, bounces=8, stats=True),
        P("f: stats() first on wide", scene="wide", spp=3, stats=True, only=INTERP),
        P("h: tiles of rank 1 of 3", tiles=(1, 3)),
        P("h: 8x8, rank 1 of 2 owns no tile", w=8, h=8, tiles=(1, 2)),
        P("h: all tiles, 40x24", spp=4),
    ]


def _generic():
    S = Step
    acc = functools.partial(S, bounces=4, group="acc")
    mom = functools.partial(S, bounces=5, group="mom", only=("simple",))
    return [
        S("a: 72x40, 5 spp", w=72, h=40, spp=5),
        S("a: down to 24x16", w=24, h=16),
        S("a: up to 64x48", w=64, h=48),
        S("a: ragged 9x17", w=9, h=17, spp=3),
        S("a: whole tiles again, 40x24"),
        S("b: 8 bounces", bounces=8),
        S("b: 0 bounces", bounces=0),
        S("b: 32 bounces", bounces=32),
        S("b: 3 bounces", spp=3),
        S("g: debug 1", bounces=8, debug=1),
        S("g: debug 3", bounces=8, debug=3),
        S("g: debug 0 again", bounces=8, spp=3),
        acc("i: 2 spp"),
        acc("i: + 2 spp on simple", kernel="simple", clear=False),
        acc("i: + 2 spp on wave", kernel="wave", clear=False),
        acc("i: + 2 spp on auto", kernel="auto", clear=False),
        mom("i: 2 spp, moments 0"),
        mom("i: + 3 spp, moments 1", moments=1, spp=3, clear=False),
        mom("i: + 2 spp, moments 0", clear=False),
        S("h: tiles of rank 1 of 3", tiles=(1, 3)),
        S("h: 8x8, rank 1 of 2 owns no tile", w=8, h=8, tiles=(1, 2)),
        S("h: all tiles, 40x24", spp=4),
    ]


WALKS = {"PIPELINE": _pipeline(), "GENERIC": _generic()}
# the transitions each walk claims (on binned_tier: those of its five steps)
CLAIMS = {"PIPELINE": "abcdefghij", "GENERIC": "abghi"}
TIER_CLAIMS = "fh"  # (and one scene change, index to table)


def units(steps):
    """The steps as the units a permutation moves: a group's steps together, every other step alone."""
    out = []
    for s in steps:
        if s.group is not None and out and out[-1][-1].group == s.group:
            out[-1].append(s)
        else:
            out.append([s])
    return out


def walk(name, seed=None, variant=None):
    """The steps of WALKS[name] that `variant` runs, in the scripted order or
    (seed) a seeded permutation of its units, each step carrying the variant."""
    variant = variant or VARIANTS[name][0]
    steps = [s for s in WALKS[name] if s.only is None or variant in s.only]
    if variant == "binned_tier":
        steps = steps[-TIER_STEPS:]
    us = units(steps)
    if seed is not None:
        random.Random(seed).shuffle(us)
    return [dataclasses.replace(s, variant=variant) for u in us for s in u]


# -- what a step is, from its data -------------------------------------------
@functools.lru_cache(maxsize=None)
def program(scene):
    return scenes.SCENES[scene]().compile(CompData())


def n_check(scene):
    return int(program(scene).n_check)


def scene_class(scene):
    """How the binned pipeline bins the scene's check[] sets (pt_bin_host.cpp plan_dispatch, ensure_bin)."""
    n = n_check(scene)
    return "index" if n <= BIN_BITS else "table" if n <= 64 else "wide"


def n_tiles(s):
    tiles = -(-s.w // TILE) * -(-s.h // TILE)
    rank, nranks = s.tiles
    return (tiles - rank + nranks - 1) // nranks if tiles > rank else 0


def full_tiles(s):
    return s.w % TILE == 0 and s.h % TILE == 0 and s.debug == 0


def kernel_of(s):
    return s.kernel or G.KERNELS[s.variant]["kernel"]


def binned(s):
    """The dispatch goes through the binned pipeline (debug 1 and 2 take the simple kernel; no tile, no launch)."""
    return kernel_of(s) == "binned" and s.debug not in (1, 2) and n_tiles(s) > 0 and s.spp > 0


@dataclasses.dataclass(frozen=True)
class Plan:
    """plan_dispatch's chunking of a binned step."""
    n_pix: int
    frames: int  # (a debug view renders the last frame only)
    per_chunk: int  # F
    lanes_used: int
    per_lane: int
    chunks: int
    passes: int
    trace_launches: int

    @property
    def need(self):
        return self.n_pix * self.per_lane


def plan(s):
    n_pix = n_tiles(s) * 64
    frames = 1 if s.debug else s.spp
    F = max(1, min(frames, s.samples // n_pix))
    lanes = min(s.lanes, F)
    launches, done = 0, 0
    while done < frames:
        fr = min(F, frames - done)
        launches += min(lanes, fr) * (s.bounces + 1)
        done += fr
    return Plan(n_pix, frames, F, lanes, -(-F // lanes), -(-frames // F), s.bounces + 1, launches)


class BinModel:
    """What ensure_bin holds after the binned launches so far: it only grows,
    reallocating everything when a launch needs more samples, passes or lanes
    (or the wide buffers for the first time)."""

    def __init__(self):
        self.cap = self.n_lanes = self.passes = 0
        self.wide = False
        self.reallocs = 0

    def launch(self, s):
        """One binned launch of step `s` (its stats() run and its dispatch plan alike); True: it reallocated."""
        p = plan(s)
        wide = scene_class(s.scene) == "wide"
        if p.need <= self.cap and p.passes <= self.passes and p.lanes_used <= self.n_lanes and (self.wide or not wide):
            return False
        self.cap, self.n_lanes = max(self.cap, p.need), max(self.n_lanes, p.lanes_used)
        self.passes = p.passes  # (the control words are sized to this launch)
        self.wide = self.wide or wide
        self.reallocs += 1
        return True

    @property
    def bin_bytes(self):
        return self.cap * self.n_lanes * (BYTES_PER_SAMPLE + (BYTES_WIDE if self.wide else 0))


# -- the transitions, computed from the steps ---------------------------------
TRANSITIONS = {
    "a": "pixels up and down: a capacity far above the live count, whole-tile and ragged sizes both ways",
    "b": "bounces 8, 0, 32, 3: the control words grow, one pass only at 0",
    "c": "bin_lanes 1, 4, 2, 3, once with fewer frames than lanes",
    "d": "bin_samples 64 (a chunk per frame) then 1 << 20 (one chunk)",
    "e": "scene changes across the bin classes, back from wide with the wide buffers allocated",
    "f": "stats() first, then the image, on a table scene (and on wide)",
    "g": "debug 1, 3, then 0",
    "h": "tiles of one rank of three, a rank that owns no tile, all tiles again",
    "i": "an accumulating group across lanes, chunk size and kernels (and one across moments)",
    "j": "two steps with the lens camera and the sky, then neither",
}


def _pairs(steps):
    return list(zip(steps, steps[1:]))


def transitions(steps, variant):
    """The letters of TRANSITIONS the steps contain, for `variant` (the
    binned-only parts of a letter count only on the PIPELINE variants; the wide
    parts of e and f only on the interpreter, the scene-kernel walk keeps to
    c1, c2 and c3)."""
    pipe = variant in VARIANTS["PIPELINE"]
    interp = variant in INTERP
    got = set()
    pairs = _pairs(steps)
    # a: sizes go down and up, whole -> ragged and ragged -> whole; binned: a live count below a quarter of the capacity
    area = [s.w * s.h for s in steps]
    shrinks = any(b < a for a, b in zip(area, area[1:])) and any(b > a for a, b in zip(area, area[1:]))
    flips = {(full_tiles(a), full_tiles(b)) for a, b in pairs if a.debug == b.debug == 0}
    far = True
    if pipe:
        m, far = BinModel(), False
        for s in steps:
            if binned(s):
                m.launch(s)
                far = far or 4 * plan(s).need < m.cap
    if shrinks and {(True, False), (False, True)} <= flips and far:
        got.add("a")
    # b: bounces up past the running maximum after the first step (ctrl grows), 0 somewhere, down again after it
    bs = [s.bounces for s in steps]
    top = bs.index(max(bs))
    if 0 in bs and top > 0 and max(bs) > max(bs[:top]) and any(b < max(bs) for b in bs[top + 1:]) and \
            {8, 0, 32, 3} <= set(bs):
        got.add("b")
    if pipe:
        if {1, 2, 3, 4} <= {s.lanes for s in steps} and \
                any(binned(s) and s.spp < s.lanes and s.lanes == 4 for s in steps):
            got.add("c")
        small = [k for k, s in enumerate(steps)
                 if binned(s) and s.samples < plan(s).n_pix and plan(s).chunks == s.spp > 1]
        if small and any(binned(s) and plan(s).chunks == 1 and s.spp > 1 and s.samples == 1 << 20
                         for s in steps[small[0] + 1:]):
            got.add("d")
        cls = {(scene_class(a.scene), scene_class(b.scene)) for a, b in pairs if a.scene != b.scene and binned(b)}
        want = {("index", "table"), ("table", "index")}
        if interp:
            want |= {("table", "wide"), ("wide", "table")}
            want_scenes = {"c2", "c3", "wide", "c3_noaabb", "cull"}
        else:
            want_scenes = {"c1", "c2", "c3"}
        if want <= cls and want_scenes <= {s.scene for s in steps}:
            got.add("e")
        fs = {scene_class(s.scene) for s in steps if s.stats and binned(s)}
        if {"table", "wide"} <= fs if interp else "table" in fs:
            got.add("f")
    # g: debug 1 -> 3 -> 0 on consecutive steps
    if any(a.debug == 1 and b.debug == 3 for a, b in pairs) and any(a.debug == 3 and b.debug == 0 for a, b in pairs):
        got.add("g")
    # h: a rank of several with tiles, a rank with none (8x8), then every tile
    if any(s.tiles[1] == 3 and n_tiles(s) > 0 for s in steps) and \
            any(n_tiles(a) == 0 and (a.w, a.h) == (8, 8) and b.tiles == (0, 1) and n_tiles(b) > 1 for a, b in pairs):
        got.add("h")
    # i: a group that goes on without a clear across kernels (binned: and lanes / chunk size)
    for u in units(steps):
        ks = [kernel_of(s) for s in u]
        if len(u) >= 4 and all(not s.clear for s in u[1:]) and u[0].clear and ks[-3:] == ["simple", "wave", "auto"]:
            if not pipe or (len(u) == 5 and (u[0].lanes, u[1].lanes, u[1].samples, u[1].spp) == (1, 3, 64, 3)):
                got.add("i")
    # j: the lens camera and the sky twice, then neither
    if any(a.sky and a.camera == "lens" and b.sky and b.camera == "lens" for a, b in pairs) and \
            any(a.sky and a.camera == "lens" and not b.sky and b.camera == "default" for a, b in pairs):
        got.add("j")
    return got


def has_moments_group(steps):
    return any([s.moments for s in u] == [0, 1, 0] and all(not s.clear for s in u[1:]) for u in units(steps))


# -- the oracle's images ------------------------------------------------------
_CHAINS = {}  # id(image) -> the render keys that made it (the images live in _render's cache)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return O.OracleScene(scenes.SCENES[name]().rows())


@functools.lru_cache(maxsize=None)
def _render(chain):
    *before, key = chain
    scene, w, h, (rank, nranks), bounces, debug, spp, sky, cam = key
    done = sum(k[6] for k in before)
    if sky or cam != "default":  # camref: pyref's loop over the oracle's map() and bounds(); whole image, cleared
        assert not before and (rank, nranks) == (0, 1)
        img = camref.render(scenes.SCENES[scene]().rows(), w, h, 1, 1, G.aspect(w, h), bounces, spp, debug,
                            camera=G.camera(cam), sky=G.sky() if sky else None)
        img = np.ascontiguousarray(img, np.float32)
    else:
        image = _render(tuple(before)).copy() if before else None
        img = _scene(scene).render(w, h, O.Constants(0.0, 1 + done, G.aspect(w, h), 1 + done),
                                   O.Settings(debug, bounces, 1.0, 1.0, 0), spp, image=image, rank=rank, nranks=nranks)
    img.setflags(write=False)
    _CHAINS[id(img)] = chain
    return img


def expected(step, carried_image=None):
    """The oracle's image after `step`: on a cleared image, or (an
    accumulating step) going on from `carried_image`, the expected image of
    the step before it, with the frame and last_clear that follow it.  Cached
    on what determines it, so the permutations of a walk share their images."""
    assert (carried_image is None) == step.clear, step.label
    before = () if carried_image is None else _CHAINS[id(carried_image)]
    return _render(before + (render_key(step),))


def frames_done(carried_image):
    """The frames already in an expected image."""
    return 0 if carried_image is None else sum(k[6] for k in _CHAINS[id(carried_image)])


@functools.lru_cache(maxsize=None)
def _counters(key):
    scene, w, h, (rank, nranks), bounces, debug, spp, _, _ = key
    return _scene(scene).render(w, h, O.Constants(0.0, 1, G.aspect(w, h), 1), O.Settings(debug, bounces, 1.0, 1.0, 0),
                                spp, rank=rank, nranks=nranks, counters=True)[1]


def expected_counters(step):
    """The oracle's work counters of a cleared step."""
    assert step.clear and not step.sky and step.camera == "default"
    return _counters(render_key(step))


def expected_images(steps):
    """[expected image after each step], the accumulating ones going on from the one before."""
    out = []
    for s in steps:
        out.append(expected(s, None if s.clear else out[-1]))
    return out


# -- running a walk on a context ----------------------------------------------
def constants(step, done=0):
    """The step's first frame after `done` frames since the clear."""
    return N.Constants(time=0.0, frame=1 + done, aspect=G.aspect(step.w, step.h), last_clear=1 + done)


def apply(pt, prev, step):
    """Make the calls that take `pt` from step `prev` to `step` (prev None:
    `pt` is open_context's fresh context, which has the scene, size, bounces
    and debug already), and clear the image for a step that starts one."""
    opts = G.KERNELS[step.variant]
    changed = (lambda f: getattr(prev, f) != getattr(step, f)) if prev is not None else (lambda f: True)
    if prev is not None and changed("scene"):
        prog = program(step.scene)
        pt.remake_pipeline(prog)
        pt.set_data(prog.data)
        G.ready(pt, opts)
    resized = prev is not None and (changed("w") or changed("h"))
    if resized:
        pt.update(resized=True, window=(step.w, step.h))
    if changed("tiles") and (prev is not None or step.tiles != (0, 1)):
        pt.set_tiles(*step.tiles)
    if prev is None or kernel_of(prev) != kernel_of(step):
        pt.set_option("kernel", kernel_of(step))
    for field, key in (("lanes", "bin_lanes"), ("samples", "bin_samples"), ("table", "bin_table")):
        if changed(field) and getattr(step, field) is not None:
            pt.set_option(key, getattr(step, field))
    if changed("moments") and (prev is not None or step.moments):
        pt.set_option("moments", step.moments)
    if changed("camera") and (prev is not None or step.camera != "default"):
        if step.camera == "default":
            pt.reset_camera()
        else:
            pt.look_at(G.EYE, G.TARGET, **G.LOOK[step.camera])
    if changed("sky") and (prev is not None or step.sky):
        if step.sky:
            pt.set_sky(**G.SKY)
        else:
            pt.clear_sky()
    pt.settings.bounces = step.bounces
    pt.settings.debug = step.debug
    if step.clear:
        pt.clear()


def open_context(step):
    """A fresh context in `step`'s configuration."""
    pt = G.tracer(step.scene, step.w, step.h, step.bounces, step.variant, debug=step.debug)
    apply(pt, None, step)
    return pt


def header_bin_bits():
    """PT_BIN_BITS as pt_binned.h has it."""
    text = (Path(N.__file__).parent / "csrc" / "pt_binned.h").read_text()
    return int(re.search(r"^#define PT_BIN_BITS (\d+)", text, re.M).group(1))
