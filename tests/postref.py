"""Shared by test_post_ref.py (no GPU), test_gpu_post_sizes.py and
test_gpu_post_reuse.py: every image-space product of a configuration -- the
image and its moments, the guides, the variance plane, the fixed and the
variance-guided filter, the history and its filter, the display pass, the
pixel queries -- from the CPU references alone (momentref, camref,
denoiseref, temporalref, rayref, oracle.display), cached by configuration and
read-only.  Also here, as data: the walk of one long-lived context through
sizes, scenes, camera moves, tiles and the moments option (WALK), a model of
the validity flags the native calls set and drop (Flags; pt_runtime.hip,
pt_post_host.cpp), and what every step of a walk must give (expectations()).
No GPU and no library state."""
import collections
import dataclasses
import functools
import random
from typing import Optional

import numpy as np

import denoiseref as D
import gpuharness as G
import momentref as MR
import rayref
import temporalref as T
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.path_tracer import look_at_camera
from compute_path_tracer_amd.sdf_editor import CompData
from oracle import oracle as O
from test_display import SPECIAL

F = np.float32
TILE = 8
TOL = dict(depth_tolerance=0.05, normal_cos=0.9, albedo_tolerance=0.1)  # test_gpu_temporal.py's

# the views by name: the reference's fixed one, test_gpu_temporal.py's A, MOVED and third view, two pans, a lens
CAMERAS = {
    "default": None,
    "A": look_at_camera(G.EYE, G.TARGET),
    "MOVED": look_at_camera((2.3, 1.4, -2.4), G.TARGET),
    "THIRD": look_at_camera((2.6, 1.3, -2.3), G.TARGET),
    "UP": look_at_camera(G.EYE, (0.0, 0.6, 0.0)),
    "FAR": look_at_camera((2.6, 1.3, -2.3), (1.0, 0.5, 0.8)),
    "lens": look_at_camera(G.EYE, G.TARGET, **G.LOOK["lens"]),
}

# A configuration.  The image is frames frame0 .. frame0 + n - 1 of `scene` under `camera` on a cleared image,
# only the tiles of rank tiles[0] of tiles[1] (the others stay zero); `view`: the camera of the guides, the
# pixel queries and the reprojection when it is not the render's (None: `camera`); `special`: test_display.py's
# special values written into the image and, rolled by 2, into the moments: from the first texel on (True) or from texel k (("at", k)).
Config = collections.namedtuple("Config", "scene w h camera frame0 n bounces tiles special view",
                                defaults=("default", 1, 3, 4, (0, 1), False, None))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


# -- scenes --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    """(program, data, rows) of a SCENES name, or of "c3-moved": c3's program
    with one shape of its first union moved by a value edit (data_update)."""
    moved = name == "c3-moved"
    ed = scenes.SCENES["c3" if moved else name]()
    cd = CompData()
    prog = ed.compile(cd)
    if moved:
        shape = ed.header_unions[0].children_shapes[0]
        shape.transform.position.set((0.7, 0.6, -0.4))
        ed.data_update(cd)
    data = np.array(cd.data_array.as_array(), np.float32)
    return prog, _frozen(data), ed.rows()


def program_of(name):
    """The SCENES name whose program (topology) the scene runs on."""
    return "c3" if name == "c3-moved" else name


# -- the image and its moments ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames(name, w, h, camera, frame0, n, bounces):
    rows = scene(name)[2]
    if camera == "default":
        return MR.oracle_frames(rows, w, h, G.aspect(w, h), bounces, n, frame0)
    return MR.camref_frames(rows, w, h, G.aspect(w, h), bounces, n, frame0, camera=CAMERAS[camera])


def owned(w, h, tiles):
    """bool (h, w): the texels of the 8x8 tiles that rank tiles[0] of tiles[1] renders."""
    rank, nranks = tiles
    ty, tx = np.arange(h)[:, None] // TILE, np.arange(w)[None, :] // TILE
    return (ty * ((w + TILE - 1) // TILE) + tx) % nranks == rank


def with_special(A, M, texel=0):
    """Copies with test_display.py's special values in A from texel `texel` (in flat order) on and, rolled by 2, in M."""
    special = np.array(SPECIAL, np.float32)
    sl = slice(4 * texel, 4 * texel + len(SPECIAL))
    assert sl.stop <= A.size
    A, M = A.copy(), M.copy()
    A.reshape(-1)[sl] = special
    M.reshape(-1)[sl] = np.roll(special, -2)
    return A, M


@functools.lru_cache(maxsize=None)
def image(cfg):
    """(A, M): the accumulation image and the moment image."""
    A, M = MR.frames_fold(_frames(cfg.scene, cfg.w, cfg.h, cfg.camera, cfg.frame0, cfg.n, cfg.bounces))
    if cfg.tiles != (0, 1):  # a texel of another rank's tile is never written: zero bits, alpha too
        own = owned(cfg.w, cfg.h, cfg.tiles)[..., None]
        A, M = np.where(own, A, F(0.0)), np.where(own, M, F(0.0))
    if cfg.special:
        A, M = with_special(A, M, 0 if cfg.special is True else cfg.special[1])
    return _frozen(np.ascontiguousarray(A, np.float32), np.ascontiguousarray(M, np.float32))


def view_camera(cfg):
    return cfg.camera if cfg.view is None else cfg.view


# -- guides, variance, the filters, display, the pixel queries -------------------------
@functools.lru_cache(maxsize=None)
def _guides(name, w, h, camera):
    return _frozen(*D.guides(scene(name)[2], w, h, G.aspect(w, h), 1.0, CAMERAS[camera]))


def guides(cfg):
    """(g0, g1) under the configuration's view (a lens as its pinhole)."""
    return _guides(cfg.scene, cfg.w, cfg.h, view_camera(cfg))


@functools.lru_cache(maxsize=None)
def variance(cfg):
    assert cfg.n >= 2
    return _frozen(MR.variance(*image(cfg), cfg.n))


@functools.lru_cache(maxsize=None)
def _denoise(cfg, params):
    return _frozen(D.atrous(image(cfg)[0], *guides(cfg), **dict(params)))


def denoise(cfg, **params):
    """pt_denoise of the image (denoiseref.atrous's defaults unless named)."""
    return _denoise(cfg, tuple(sorted(params.items())))


@functools.lru_cache(maxsize=None)
def _guided(cfg, params):
    return _frozen(MR.guided(image(cfg)[0], variance(cfg), *guides(cfg), **dict(params)))


def denoise_guided(cfg, **params):
    """pt_denoise_guided of the image (momentref.guided's defaults unless named)."""
    return _guided(cfg, tuple(sorted(params.items())))


def display(img):
    """(RGBA32F, sRGB8): the display pass of a linear image in both formats."""
    img = np.ascontiguousarray(img, np.float32)
    return O.display(img), O.display(img, srgb8=True)


@functools.lru_cache(maxsize=None)
def _picks(name, w, h, camera):
    xy = [(x, y) for y in range(h) for x in range(w)]
    t, node, nrm = rayref.pick(scene(name)[2], w, h, G.aspect(w, h), 1.0, CAMERAS[camera], xy)
    return _frozen(t.reshape(h, w), node.reshape(h, w), nrm.reshape(h, w, 3))


def picks(cfg):
    """rayref.pick of every pixel: (t (h, w), node (h, w), normal (h, w, 3))."""
    return _picks(cfg.scene, cfg.w, cfg.h, view_camera(cfg))


# -- the history -------------------------------------------------------------------
def view_of(cfg):
    return T.View(CAMERAS[view_camera(cfg)], G.aspect(cfg.w, cfg.h), 1.0)


def accumulate(cfg, hist, cap):
    """(History, counts): the configuration's view merged into `hist` (None: no history held)."""
    A, M = image(cfg)
    hist, counts = T.accumulate(A, M, *guides(cfg), cfg.n, view_of(cfg), hist, cap, **TOL)
    _frozen(hist.colour, hist.moments, hist.count)
    return hist, counts


@functools.lru_cache(maxsize=None)
def _history(chain):
    *before, (cfg, cap) = chain
    return accumulate(cfg, _history(tuple(before))[0] if before else None, cap)


def history(chain):
    """(History, counts) after the accumulates chain = ((cfg, max_history), ...) from no history, cached by the chain."""
    return _history(tuple(chain))


def denoise_history(hist, **params):
    return T.denoise_history(hist, **params)


def history_planes(hist):
    return hist.colour, hist.moments, hist.count


# -- the edge sizes of test_gpu_post_sizes.py ----------------------------------------
# size -> what it is the smallest case of
SIZES = {
    (1, 1): "no neighbour at any step; one thread of one block",
    (1, 40): "one column: every tap of the x axis outside, x0 + 1 always outside",
    (40, 1): "one row: every tap of the y axis outside, y0 + 1 always outside",
    (3, 2): "smaller than the step-1 halo in both axes",
    (16, 16): "exactly one LDS tile, a quarter of a direct block wide",
    (17, 33): "one past the LDS tile in x, one past two tiles in y, one past eight 4-row direct blocks",
    (64, 4): "exactly one direct / temporal block",
    (65, 5): "one past one direct / temporal block in both axes",
    (128, 8): "whole blocks only in both forms: no ragged edge, interior LDS tiles with a full halo",
}
FIXED_ITERATIONS = (1, 2, 5, 8)  # even and odd counts: both result buffers; 8: step 128, at or beyond every size
GUIDED_ITERATIONS = (5, 8)
TEMPORAL_VIEWS = ("A", "A", "MOVED")  # the views of test_gpu_temporal.py's special-value case
PICK_TEXELS = 17 * 33  # rayref.pick of every pixel up to this size


def size_config(w, h):
    """c2 under the reference's fixed view, 3 frames, 4 bounces; the special values from 64 texels on."""
    return Config("c2", w, h, "default", 1, 3, 4, (0, 1), w * h >= 64)


def temporal_chain(w, h, special=False):
    """The accumulates of a size's temporal run: c3 at 4 frames per view,
    frames of its own for each, caps of 32.  special: the special values
    written as test_gpu_temporal.py's _special_case writes them -- into the
    first view, so they enter the history, and elsewhere into the second,
    whose taps land on the first's -- but over the first and the last run of
    four hit texels of the view (the corners of these flat images miss, and a
    miss neither reads a history texel nor counts as not finite).  The image and moments are the
    fixed camera's (the C oracle renders them; the Python path tracer a posed
    render needs takes about a millisecond per sample), the guides and the reprojection
    the views': the accumulate reads colours and guides and never asks
    whether one camera made both."""
    where = (False, False, False)
    if special:
        hit = _guides("c3", w, h, TEMPORAL_VIEWS[0])[1][..., 3].reshape(-1) != 0
        runs = [k for k in range(w * h - 3) if hit[k:k + 4].all()]
        assert runs and runs[-1] >= runs[0] + 4 and TEMPORAL_VIEWS[0] == TEMPORAL_VIEWS[1]
        where = (("at", runs[0]), ("at", runs[-1]), False)
    return tuple((Config("c3", w, h, "default", 1 + 16 * k, 4, 4, (0, 1), where[k], view), 32.0)
                 for k, view in enumerate(TEMPORAL_VIEWS))


# -- the walk of test_gpu_post_reuse.py ----------------------------------------------
@dataclasses.dataclass(frozen=True)
class Step:
    """An absolute description of the context and of what to render, so a walk
    can run in any order: apply() of test_gpu_post_reuse.py makes only the
    calls that take a context from one step to the next (calls())."""
    label: str
    scene: str = "c3"
    w: int = 24
    h: int = 16
    camera: str = "default"
    frame0: int = 1
    n: int = 3
    tiles: tuple = (0, 1)
    moments: int = 1
    cap: float = 32.0  # max_history of the step's accumulate
    orders: bool = False  # the three users of mom.var in every order, denoise() between two guided calls
    group: Optional[str] = None  # steps of one group move as one unit

    @property
    def cfg(self):
        return Config(self.scene, self.w, self.h, self.camera, self.frame0, self.n, BOUNCES, self.tiles)


BOUNCES = 4
SEED = 3  # (an order whose neighbouring steps accumulate different frame counts: the count planes differ)
KERNELS = ("binned_jit", "simple")


def _walk():
    S = Step
    b = functools.partial(S, w=20, h=12, group="b")
    c = functools.partial(S, w=16, h=10, group="c")
    d = functools.partial(S, group="d")
    f = functools.partial(S, group="f")
    steps = [
        S("a: c3 at 61x37", w=61, h=37),
        S("a: shrink to 24x16: the capacity stays", n=4),
        S("a: grow to 72x40: everything reallocated", w=72, h=40, n=2),
        S("a: 40x72: the same texel count, another stride", w=40, h=72),
        S("a: ragged 9x17", w=9, h=17, n=4),
        b("b: c3 at 20x12", n=2),
        b("b: c2 through remake_pipeline + set_data", scene="c2"),
        b("b: back to c3", n=4),
        b("b: a value edit moves a shape", scene="c3-moved", n=2),
        c("c: view A", camera="A", n=3),
        c("c: the view panned up, the history carried along", camera="UP", n=2),
        c("c: the eye moved and the view panned, cap 3", camera="FAR", n=3, cap=3.0),
        c("c: clear at the same size: the history stays", camera="FAR", n=4),
        c("c: a resize drops the history", camera="FAR", w=12, h=8, n=2),
        d("d: all tiles"),
        d("d: tiles of rank 1 of 3", tiles=(1, 3), n=4),
        d("d: all tiles again", n=2),
        d("e: the users of mom.var in every order", orders=True),
        f("f: moments off", moments=0, n=2),
        f("f: moments on", n=4),
        S("f: a lens camera", camera="lens", w=12, h=8, n=2),
    ]
    # every step renders frames of its own
    return [dataclasses.replace(s, frame0=1 + 16 * k) for k, s in enumerate(steps)]


WALK = _walk()
CLAIMS = "abcdef"
TRANSITIONS = {
    "a": "shrink below the capacity, grow past it, the same texel count with another stride, a ragged size",
    "b": "a scene through remake_pipeline + set_data at the same size, a value edit, back again",
    "c": "three views with the history carried along (caps 32 and 3), a clear at the same size, a resize",
    "d": "tiles of one rank of three, then every tile",
    "e": "the three users of mom.var in every order, on a context that holds a history",
    "f": "moments off and on again; a lens camera",
}


def units(steps):
    out = []
    for s in steps:
        if s.group is not None and out and out[-1][-1].group == s.group:
            out[-1].append(s)
        else:
            out.append([s])
    return out


def walk(seed=None):
    """WALK in the scripted order, or (seed) in a seeded permutation of its units."""
    us = units(WALK)
    if seed is not None:
        random.Random(seed).shuffle(us)
    return [s for u in us for s in u]


def iterations(k):
    """The iteration count of step k's filters: odd and even alternate, so both result buffers serve."""
    return 5 if k % 2 == 0 else 4


def lds(k):
    """denoise_lds of step k: two steps off, two steps on."""
    return (k // 2) % 2


class Flags:
    """What the native calls do to the validity flags (pt_runtime.hip,
    pt_post_host.cpp, pt_options.cpp): guides (dn.guides_valid), history
    (hist.valid) and its count of
    accumulates (hist.views), moments (mom.valid)."""

    def __init__(self):
        self.guides = self.history = self.moments = False
        self.views = 0  # hist.views: the accumulates since the history was last dropped

    def on(self, call):
        if call in ("remake_pipeline", "set_data"):
            self.guides = self.history = False
            self.views = 0
        elif call == "resize":  # pt_resize_clear to another size
            self.guides = self.history = self.moments = False
            self.views = 0
        elif call == "clear":  # pt_resize_clear to the same size: the history stays
            self.guides = self.moments = False
        elif call in ("set_tiles", "set_moments"):  # (pt_set_tiles keeps the guides and the history)
            self.moments = False
        elif call == "set_camera":
            self.guides = False
        elif call == "dispatch_moments":  # a dispatch from last_clear 0 with the option on
            self.moments = True
        elif call == "dispatch":
            self.moments = False
        elif call == "render_guides":
            self.guides = True
        elif call == "accumulate":
            self.history = True
            self.views += 1
        else:
            raise ValueError(call)


def calls(prev, step):
    """The calls that take a context from step `prev` to `step`, in order (prev
    None: a fresh context that has the scene, the size and moments on), before
    the clear that starts every step."""
    out = []
    if prev is None:
        if step.camera != "default":
            out.append("set_camera")
        if step.tiles != (0, 1):
            out.append("set_tiles")
        if not step.moments:
            out.append("set_moments")
        return out
    if program_of(prev.scene) != program_of(step.scene):
        out += ["remake_pipeline", "set_data"]
    elif prev.scene != step.scene:
        out.append("set_data")
    if (prev.w, prev.h) != (step.w, step.h):
        out.append("resize")
    if prev.tiles != step.tiles:
        out.append("set_tiles")
    if prev.camera != step.camera:
        out.append("set_camera")
    if prev.moments != step.moments:
        out.append("set_moments")
    return out


@dataclasses.dataclass
class Expect:
    """What step k of a walk must give."""
    step: Step
    k: int
    calls: list
    before: Flags  # after the transition's calls and the clear, before the render
    history_before: Optional[T.History]  # the history held then (None: none valid)
    products: dict  # name -> array, every product the step can form
    counts: Optional[dict]  # the accumulate's counts (None: refused)
    history: Optional[T.History]  # the history held after the step


def accumulates(step):
    return bool(step.moments) and step.tiles == (0, 1)


def expectations(steps):
    """[Expect] of the steps in their order, the reference history carried beside the flags."""
    out, flags, hist, prev = [], Flags(), None, None
    for k, s in enumerate(steps):
        made = calls(prev, s)
        for call in made:
            flags.on(call)
        flags.on("clear")
        before = Flags()
        before.__dict__.update(flags.__dict__)
        held = hist if flags.history else None
        cfg, it = s.cfg, iterations(k)
        A, M = image(cfg)
        g0, g1 = guides(cfg)
        p = {"A": A, "g0": g0, "g1": g1, "fixed": denoise(cfg, iterations=it)}
        flags.on("dispatch_moments" if s.moments else "dispatch")
        flags.on("render_guides")
        counts = None
        if s.moments:
            p.update(M=M, V=variance(cfg), guided=denoise_guided(cfg, iterations=it))
        if accumulates(s):
            hist, counts = accumulate(cfg, held, s.cap)
            flags.on("accumulate")
        else:
            hist = held
        if flags.history:
            p.update(hc=hist.colour, hm=hist.moments, hn=hist.count, hfiltered=denoise_history(hist, iterations=it))
        out.append(Expect(s, k, made, before, held, p, counts, hist if flags.history else None))
        prev = s
    return out


def transitions(steps):
    """The letters of TRANSITIONS the steps contain, from the step data and the flags' model."""
    got = set()
    ex = expectations(steps)
    pairs = list(zip(steps, steps[1:]))
    area = [s.w * s.h for s in steps]
    top = [max(area[:k + 1]) for k in range(len(area))]
    shrink = any(b < a for a, b in zip(area, area[1:]))
    grow = any(area[k] > top[k - 1] for k in range(1, len(area)))
    same_count = any(a.w * a.h == b.w * b.h and a.w != b.w and e.history_before is None and e.counts is not None and
                     e.counts["no_history"] == b.w * b.h for (a, b), e in zip(pairs, ex[1:]))
    ragged = any(s.w % TILE and s.h % TILE and s.w % 16 and s.h % 4 for s in steps)
    if shrink and grow and same_count and ragged:
        got.add("a")
    size = lambda s: (s.w, s.h)  # noqa: E731
    if any(e.calls[:2] == ["remake_pipeline", "set_data"] and size(a) == size(b) for (a, b), e in zip(pairs, ex[1:])) and \
            any(e.calls == ["set_data"] for e in ex[1:]) and \
            any(a.scene == "c2" and b.scene == "c3" for a, b in pairs):
        got.add("b")
    moved = [e for (a, b), e in zip(pairs, ex[1:]) if "set_camera" in e.calls and e.history_before is not None and
             e.counts is not None and 0 < e.counts["taken"]]
    kept = [e for e in ex[1:] if not e.calls and e.history_before is not None and e.counts and e.counts["taken"] > 0]
    dropped = [e for (a, b), e, p in zip(pairs, ex[1:], ex) if p.history is not None and "resize" in e.calls and
               e.history_before is None and e.counts and e.counts["no_history"] == b.w * b.h]
    if len(moved) >= 2 and {32.0, 3.0} <= {e.step.cap for e in moved} and kept and dropped:
        got.add("c")
    if any(a.tiles == (0, 1) and b.tiles[1] == 3 and e.before.history and e.counts is None and e.history is not None
           for (a, b), e in zip(pairs, ex[1:])) and any(a.tiles[1] == 3 and b.tiles == (0, 1) for a, b in pairs):
        got.add("d")
    if any(e.step.orders and e.history is not None and e.step.moments for e in ex):
        got.add("e")
    if any(not a.moments and b.moments for a, b in pairs) and any(s.camera == "lens" for s in steps):
        got.add("f")
    return got


STALE = ("g0", "g1", "V", "fixed", "guided", "hc", "hm", "hn", "hfiltered")


def stale_shares(ex):
    """Of each product of each step, against the array the step before left
    of it: (product, step, the step that left it, the share of floats that
    differ over the common flat prefix).  Left out, because there the old bits
    are the right answer: guides of an unchanged scene, size and view (the
    same cached arrays), and the history of a step whose accumulate is refused."""
    left = {}
    for e in ex:
        for name in STALE:
            new = e.products.get(name)
            if new is None:
                continue
            old, by = left.get(name, (None, None))
            left[name] = (new, e.step.label)
            if old is None or new is old or (name.startswith("h") and e.counts is None):
                continue
            n = min(old.size, new.size)
            yield name, e.step.label, by, float(np.mean(G.bits(old).reshape(-1)[:n] != G.bits(new).reshape(-1)[:n]))
