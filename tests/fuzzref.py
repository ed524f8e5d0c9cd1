"""Shared by test_scene_fuzz.py (no GPU) and test_gpu_fuzz.py: the census of
what a set of random scenes holds, the oracle images they are compared with,
and the live-edit sequence on C3.  No GPU and no library state of its own."""
import functools
import math
import re

import numpy as np

from compute_path_tracer_amd import _native as N, scenes
from compute_path_tracer_amd.sdf_editor import CompData
from gpuharness import aspect, first_difference, oracle_image, pixels_changed  # noqa: F401 (used as R.<name>)

# the size every random scene is rendered at on the GPU
W, H, SPP, BOUNCES = 24, 16, 2, 4
KINDS = {N.PT_NODE_SPHERE: "sphere", N.PT_NODE_CUBE: "cube", N.PT_NODE_TORUS: "torus",
         N.PT_NODE_OCTAHEDRON: "octahedron"}
ROLES = {N.PT_COMBINE_ASSIGN: "first", N.PT_COMBINE_UNION: "union-member", N.PT_COMBINE_SUBTRACTION: "sub-member"}


@functools.lru_cache(maxsize=None)
def fuzz_oracle(seed, profile="mixed", w=W, h=H, spp=SPP, bounces=BOUNCES):
    """The oracle's image of fuzz_scene(seed, profile), computed once and shared (read-only)."""
    img = oracle_image(scenes.fuzz_scene(seed, profile), w, h, spp, bounces)
    img.setflags(write=False)
    return img


def _literal(tok):
    """One number of a baked PtNode literal (pt_jit.cpp hexf)."""
    tok = tok.strip()
    if tok.startswith("__builtin_nanf"):
        return math.nan
    if tok.startswith("(-__builtin_inff"):
        return -math.inf
    if tok.startswith("__builtin_inff"):
        return math.inf
    if tok.endswith("u"):
        return float(int(tok[:-1]))
    if tok.startswith("0x") or tok.startswith("-0x"):
        return float.fromhex(tok.rstrip("f"))
    return float(tok.rstrip("f"))


def baked_map(prog, data=None):
    """The first map (JitMap) of the values-baked source: generated, not compiled."""
    src = N.scene_kernel_source(prog, data=data, baked=1)
    return src[:src.index("struct JitMapB")]


def union_pads(prog, src=None):
    """PtNode.pad[0] of every UNION_BEGIN (pt_derive.cpp pt_cull_bounds: the
    union's 1/s when its cull rule is on, NaN when it is off), read from the
    values-baked source's node literals as test_cull.py does."""
    pads = []
    for m in re.finditer(r"constexpr PtNode B\d+\{(.*?)\};\n", src if src is not None else baked_map(prog)):
        toks = [t for t in m.group(1).replace("{", ",").replace("}", ",").split(",") if t.strip()]
        if int(_literal(toks[0])) == N.PT_OP_UNION_BEGIN:
            pads.append(_literal(toks[19]))
    return pads


def baked_fast_bounds(prog, data=None):
    """pt_fast_bounds as the values-baked bounds() carries it."""
    src = N.scene_kernel_source(prog, data=data, baked=1)
    fast, slow = "const bool fast = true && " in src, "const bool fast = false && " in src
    assert fast != slow
    return fast


def features(ed):
    """The set of fuzz_scene's documented features this scene holds, from
    rows(), op_dicts() and the values-baked source (union bounds, cube paths)."""
    rows, prog = ed.rows(), ed.compile(CompData())
    f = set()
    for o in prog.op_dicts():
        if o["opcode"] == N.PT_OP_SHAPE:
            f.add(f"{KINDS[o['shape']]} as {ROLES[o['combine']]}")
    kids = {i: [] for i, r in enumerate(rows) if r["kind"] == N.PT_NODE_UNION}
    depth, world = {}, {}
    for i, r in enumerate(rows):
        p = r["parent"]
        if p >= 0:
            kids[p].append(i)
        up = world[p] if p >= 0 else 1.0
        world[i] = up * r["scale"]
        if r["kind"] == N.PT_NODE_UNION:
            depth[i] = depth[p] + 1 if p >= 0 else 1
            if p < 0:
                f.add("header Subtraction" if r["union_type"] == N.PT_UNION_TYPE_SUBTRACTION else "header Union")
            if r["scale"] != 1.0:
                f.add("union scale not 1")
            if not 0.5 <= r["scale"] <= 2.0:
                f.add("union scale outside [1/2, 2]")
        else:
            s = r["scale"]
            f.add("shape scale 0.5" if s == 0.5 else "shape scale 2" if s == 2.0 else
                  "shape scale 1" if s == 1.0 else "shape scale non-dyadic" if math.frexp(s)[0] != 0.5 else "")
            f.add("box on" if r["aabb"] else "box off")
            if r["aabb"]:
                for ex in (1.0, 1.3, 2.0):
                    if r["aabb_exaggeration"] == float(np.float32(ex)):
                        f.add(f"exaggeration {ex}")
            spec = r["material"][7]
            f.add("specular 0" if spec == 0.0 else "specular 1" if spec == 1.0 else "specular fractional")
            if r["material"][3] > 0.0:
                f.add("emitter")
        # the identity flags of pt_derive.cpp (PT_NF_*)
        f.add("scale 1" if r["scale"] == 1.0 else "scale not 1")
        f.add("position 0" if all(v == 0.0 for v in r["position"]) else "position not 0")
        for k, ax in enumerate("xyz"):
            f.add(f"rotation {ax} 0" if r["rotation"][k] == 0.0 else f"rotation {ax} not 0")
    for i, c in kids.items():
        if not c:
            f.add("empty union")
        elif all(rows[k]["kind"] == N.PT_NODE_UNION for k in c):
            f.add("union with only child unions")
    if depth and max(depth.values()) >= 3:
        f.add("nesting depth >= 3")
    src = baked_map(prog)
    for p in union_pads(prog, src):
        f.add("cull rule off" if math.isnan(p) else "cull rule on")
    # which cubes the generator gives the one-face path (pt_jit.cpp fast_cube), as it wrote them
    if "sdf_k<%d, true>(" % N.PT_NODE_CUBE in src:
        f.add("cube fast")
    if "sdf_k<%d>(" % N.PT_NODE_CUBE in src:
        f.add("cube not fast")
    f.discard("")
    return f


WANTED = ({f"{k} as {r}" for k in KINDS.values() for r in ROLES.values()} |
          {"header Union", "header Subtraction", "nesting depth >= 3", "empty union", "union with only child unions",
           "scale 1", "scale not 1", "position 0", "position not 0", "rotation x 0", "rotation x not 0", "rotation y 0",
           "rotation y not 0", "rotation z 0", "rotation z not 0", "shape scale 0.5", "shape scale 2",
           "shape scale non-dyadic", "union scale not 1", "union scale outside [1/2, 2]", "box on", "box off", "exaggeration 1.0",
           "exaggeration 1.3", "exaggeration 2.0", "cube fast", "cube not fast", "emitter", "specular 0",
           "specular fractional", "specular 1", "cull rule on", "cull rule off"})


# -- the live-edit sequence on C3 (32x20, 2 spp, 4 bounces) -----------------
EW, EH, ESPP, EBOUNCES = 32, 20, 2, 4


def _sh(ed, u, s):
    return ed.header_unions[u].children_shapes[s]


def _set(get, value):
    """An edit that stores `value` (one number, or three for a V3 / a cube's
    size) and returns the inverse edit's value."""
    def run(ed):
        t = get(ed)
        if isinstance(t, list):  # a cube's three size Floats
            old = [p.val for p in t]
            for p, v in zip(t, value):
                p.set(v)
        elif hasattr(t, "vals"):
            old = t.vals()
            t.set(value)
        else:
            old = t.val
            t.set(value)
        return old

    return run


# (label, target, value, undo, changes the table source[, (fast_bounds, bound_k
# is finite) after the edit: what pt_set_data derives, (True, True) otherwise
# and after every inverse])
# Shapes the fixed camera sees: objects-a-4 (sphere), objects-a-6 (emissive
# cube), objects-a-2 (cube), objects-c-0, objects-b-0 (boxed cubes), the room's light and wall "7".
# undo: the next step puts the old value back, and must restore the earlier
# oracle image bit for bit.
EDITS = [
    ("boxed sphere position x to 1e20: fast_bounds off, bound_k NaN",
     lambda ed: _sh(ed, 1, 4).transform.position.x, 1e20, True, False, (False, False)),
    ("boxed sphere position y to NaN: every coordinate of the sphere is NaN, its box ignores y",
     lambda ed: _sh(ed, 1, 4).transform.position.y, float("nan"), True, False, (False, False)),
    ("boxed cube position y to 3e6: bound_k NaN only",
     lambda ed: _sh(ed, 3, 0).transform.position.y, 3e6, True, False, (True, False)),
    ("cube size y to -0.1 in objects-a, whose cull rule is on: the rule goes off",
     lambda ed: _sh(ed, 1, 6).current_shape.params[1], -0.1, True, False),
    ("sphere radius to -0.2",
     lambda ed: _sh(ed, 1, 4).current_shape.params[0], -0.2, True, False),
    ("brightness of the non-emitting wall '7' to 5",
     lambda ed: _sh(ed, 0, 4).material.brightness, 5.0, False, False),
    ("the room light's light colour to (0, 0, 0): NaN emission",
     lambda ed: _sh(ed, 0, 2).material.light_col, (0.0, 0.0, 0.0), True, False),
    ("box exaggeration of objects-b-0 to 0",
     lambda ed: _sh(ed, 2, 0).transform.aabb_exaggeration, 0.0, True, False),
]
# C3 has no shape with a scale other than 1, so one leaves 1 first (an identity
# flag flips: a new scene kernel source, one compile), then goes on to 1e-7 and
# back within that source
EDITS_SCALE = [
    ("shape scale of objects-a-6 from 1 to 0.8: PT_NF_SCALE sets",
     lambda ed: _sh(ed, 1, 6).transform.scale, 0.8, False, True),
    ("that shape's scale, now other than 1, to 1e-7: its bound is NaN, the union's rule goes off",
     lambda ed: _sh(ed, 1, 6).transform.scale, 1e-7, True, False, (True, False)),
]
# a union's scale is part of the source (its shapes' world scale), so this one
# is for the interpreter kernels, which compile nothing: bound_k NaN
EDITS_INTERPRETER = [
    ("scale 1.1 of union objects-c to 1e-7",
     lambda ed: ed.header_unions[3].transform.scale, 1e-7, True, True, (True, False)),
]
# the two that change the source (one compile each on a scene kernel)
EDITS_SOURCE = [
    ("rotation x of objects-c-0 to exactly 0: PT_NF_RX clears",
     lambda ed: _sh(ed, 3, 0).transform.rotation.x, 0.0, False, True),
    ("cube objects-a-2 across the fast_cube threshold (middle half-extent 0.448 -> 1.1)",
     lambda ed: _sh(ed, 1, 2).current_shape.params, (1.2, 1.1, 0.448), False, True),
]


def edit_steps(edits):
    """[(label, run(ed), changes_source, restores, (fast_bounds, bound_k is
    finite))]: every edit, each with undo followed at once by its inverse;
    `restores` marks an inverse, whose oracle image must equal the one before
    the edit."""
    steps = []
    for label, get, value, undo, src, *state in edits:
        box = {}
        state = state[0] if state else (True, True)

        def do(ed, get=get, value=value, box=box):
            box["old"] = _set(get, value)(ed)

        steps.append((label, do, src, False, state))
        if undo:
            def back(ed, get=get, box=box):
                _set(get, box["old"])(ed)

            steps.append(("back: " + label, back, src, True, (True, True)))
    return steps


# -- programs at pt_set_program's limits ------------------------------------
def boxed_scene(n):
    """`n` small boxed shapes (so n check[] entries: 128 is PT_MAX_CHECK) in
    unions of 16, on a grid the fixed camera sees; every second one glows."""
    unions = []
    for k in range(n):
        if k % 16 == 0:
            unions.append(scenes._union(f"grid-{k // 16}", pos=(0.0, 0.0, 0.25 * (k // 16))))
        col, row = k % 16, k // 16
        kind = (scenes.Shapes.SPHERE, scenes.Shapes.CUBE, scenes.Shapes.OCTAHEDRON)[k % 3]
        size = (0.2, 0.15, 0.18) if kind == scenes.Shapes.CUBE else (0.2,)
        s = scenes._shape(kind, pos=(-3.0 + 0.4 * col, -1.6 + 0.4 * row, 0.5), rot=(0.1 * col, 0.0, 0.05 * row),
                          size=size, name=f"grid-{k}")
        scenes._mat(s, col=(0.3 + 0.04 * col, 0.8, 0.9 - 0.04 * col), brightness=2.0 if k % 2 == 0 else 0.0,
                    spec=0.5 if k % 5 == 0 else 0.0, rough=0.2)
        unions[-1].children_shapes.append(s)
    return scenes.SDFEditor(unions)


def chain_scene(levels):
    """A chain of unions nested `levels` deep with a shape at every level
    (8 is PT_MAX_DEPTH); the outermost shape glows."""
    top = parent = None
    for d in range(levels):
        u = scenes._union(f"level-{d}", pos=(0.1, 0.0, 0.0), rot=(0.0, 0.1 * d, 0.0), scale=1.0 if d % 2 else 0.9)
        s = scenes._shape(scenes.Shapes.SPHERE if d % 2 else scenes.Shapes.CUBE, pos=(-1.0 + 0.3 * d, 0.2, 0.5),
                          size=(0.6, 0.5, 0.4) if d % 2 == 0 else (0.6,), aabb=False, name=f"level-{d}-0")
        scenes._mat(s, col=(0.8, 0.5, 0.3), brightness=2.0 if d == 0 else 0.0)
        u.children_shapes.append(s)
        if parent is None:
            top = u
        else:
            parent.children_unions.append(u)
        parent = u
    return scenes.SDFEditor([top])

