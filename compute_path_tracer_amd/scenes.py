"""Synthetic scenes for BASELINE.json's configurations.

All scenes are built through the editor mirror (:mod:`.sdf_editor`) so they
exercise the same compile path a user scene takes.  Values are deterministic.

* ``c1_default`` -- the editor's default scene (sdf_editor.rs:26-27: one Union
  holding one unit Sphere, AABB on, exaggeration 1.3) with brightness 1 so the
  image is not black (the default Material has brightness 0).
* ``c2_sphere_box_torus`` -- (sphere U box) - torus expressed in the
  reference's union semantics: header union A (Subtraction) = [torus, sphere]
  -> sphere - torus; header union B (Subtraction) = [torus, box] -> box -
  torus; the header level always unions, giving (sphere U box) - torus.  Plus
  one emissive sphere.  The torus is a build extension (absent upstream).
* ``c3_graph32`` -- a flat 32-node graph: 4 header unions x 7 shapes.  Union 0
  is the Cornell-like room of the reference's saved scene assets/maps/test.json
  (floor, roof, emissive light box, tilted back wall, two side walls; values
  copied, light colour (0,0,0) of non-emitters replaced by the live editor's
  default (1,1,1) because the current Mat normalises it), plus the two
  rough-specular octahedra of that file in union 1; the rest is drawn from a
  fixed PRNG (seed 42): spheres/cubes, sizes in [0.2, 0.75], rotations in
  [-pi, pi]; unions 1-3 mix Union/Subtraction and carry their own transforms.
  AABB culling is on for 24 of the 28 shapes.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np

from .sdf_editor import SDFEditor, Shape, Shapes, Union, UnionType


def _mat(shape: Shape, col=(1, 1, 1), brightness=0.0, light=(1, 1, 1), spec=0.0, spec_col=(1, 1, 1), rough=0.0):
    m = shape.material
    m.color.set(col)
    m.brightness.set(brightness)
    m.light_col.set(light)
    m.specular_chance.set(spec)
    m.specular_color.set(spec_col)
    m.roughness.set(rough)


def _shape(kind: str, pos=(0, 0, 0), rot=(0, 0, 0), scale=1.0, size: Sequence[float] = (1.0,), aabb=True, name="Shape",
           ex=1.3) -> Shape:
    s = Shape(kind)
    s.name = name
    s.transform.position.set(pos)
    s.transform.rotation.set(rot)
    s.transform.scale.set(scale)
    s.transform.aabb = aabb
    s.transform.aabb_exaggeration.set(ex)
    for p, v in zip(s.current_shape.params, size):
        p.set(v)
    return s


def _union(name: str, union_type=UnionType.UNION, pos=(0, 0, 0), rot=(0, 0, 0), scale=1.0) -> Union:
    u = Union(union_type)
    u.name = name
    u.transform.position.set(pos)
    u.transform.rotation.set(rot)
    u.transform.scale.set(scale)
    return u


def empty() -> SDFEditor:
    """PLACEHOLDER_MAP (state.rs:20-36): no unions; every pixel misses."""
    return SDFEditor([])


def c1_default() -> SDFEditor:
    ed = SDFEditor()  # Union + Sphere(1.0), defaults everywhere
    _mat(ed.header_unions[0].children_shapes[0], brightness=1.0)
    return ed


def c2_sphere_box_torus() -> SDFEditor:
    torus_rot = (1.2, 0.3, 0.0)

    def torus():
        t = _shape(Shapes.TORUS, pos=(0.0, 0.0, 0.2), rot=torus_rot, size=(1.05, 0.32), name="torus")
        _mat(t, col=(0.15, 0.35, 0.95), spec=0.2, rough=0.4)
        return t

    a = _union("sphere-torus", UnionType.SUBTRACTION)
    a.children_shapes.append(torus())
    sph = _shape(Shapes.SPHERE, pos=(-0.75, 0.0, 0.3), size=(0.95,), name="sphere")
    _mat(sph, col=(0.9, 0.25, 0.2))
    a.children_shapes.append(sph)

    b = _union("box-torus", UnionType.SUBTRACTION)
    b.children_shapes.append(torus())
    box = _shape(Shapes.CUBE, pos=(0.8, -0.1, 0.2), rot=(0.3, 0.6, 0.1), size=(0.7, 0.7, 0.7), name="box")
    _mat(box, col=(0.85, 0.85, 0.8), spec=0.5, spec_col=(1.0, 0.9, 0.7), rough=0.25)
    b.children_shapes.append(box)

    light = _union("light")
    ls = _shape(Shapes.SPHERE, pos=(0.0, 3.2, -0.5), size=(1.2,), name="light")
    _mat(ls, col=(1, 1, 1), brightness=4.0)
    light.children_shapes.append(ls)
    floor = _shape(Shapes.CUBE, pos=(0.0, -2.0, 1.0), size=(6.0, 0.5, 6.0), name="floor")
    _mat(floor, col=(0.6, 0.6, 0.6), spec=0.1, rough=0.6)
    light.children_shapes.append(floor)
    return SDFEditor([a, b, light])


# assets/maps/test.json (deprecated node-editor save of the reference)
_ROOM = [
    ("floor", (11.63, 1.0, 12.26), (0.0, -2.32, 0.0), (0.0, 0.0, 0.0),
     dict(col=(0.0, 0.6313726, 1.0), spec=0.75, spec_col=(0.50980395, 0.53333336, 1.0), rough=0.2)),
    ("roof", (11.63, 1.0, 12.26), (0.0, 3.25, 0.0), (0.0, 0.0, 0.0),
     dict(col=(0.0, 0.2509804, 1.0), spec=0.0, spec_col=(0.0, 0.0, 0.0), rough=0.0)),
    ("light", (1.0, 1.0, 2.0), (0.0, 3.23, 1.85), (0.0, 0.0, 0.0),
     dict(col=(0.0, 0.0, 0.0), brightness=1.2, light=(1.0, 1.0, 1.0), spec=0.0, spec_col=(0.0, 0.0, 0.0))),
    ("4", (11.63, 1.0, 12.26), (0.0, 3.25, 3.75), (1.4, 0.0, 0.0),
     dict(col=(1.0, 0.0, 0.0), spec=0.0, spec_col=(0.0, 0.0, 0.0))),
    ("7", (1.0, 1.15, 7.2), (3.0, 0.0, 2.1), (0.0, -0.22, 0.0),
     dict(col=(0.0, 0.0, 0.0), spec=0.5, spec_col=(1.0, 1.0, 1.0))),
    ("8", (1.0, 1.15, 7.2), (-3.0, 0.0, 2.1), (0.0, 0.22, 0.0),
     dict(col=(0.0, 0.0, 0.0), spec=0.5, spec_col=(1.0, 1.0, 1.0))),
]
_OCTA = [
    ("5", 1.0, (0.0, -0.06, 1.8), (1.61, 2.82, 1.87)),
    ("6", 1.0, (-0.05, -0.2, 1.8), (1.7, 1.8, 2.68)),
]


def c3_graph32(seed: int = 42) -> SDFEditor:
    rng = np.random.default_rng(seed)
    room = _union("room")
    for name, size, pos, rot, mat in _ROOM:
        s = _shape(Shapes.CUBE, pos=pos, rot=rot, size=size, name=name, aabb=name not in ("floor", "roof"))
        _mat(s, **mat)
        room.children_shapes.append(s)
    # 7th room piece: a small emissive panel on the left wall
    panel = _shape(Shapes.CUBE, pos=(-1.9, 1.2, 3.0), rot=(0.0, 0.22, 0.0), size=(0.05, 0.4, 0.8), name="panel")
    _mat(panel, col=(1, 1, 1), brightness=2.5, light=(1.0, 0.85, 0.6))
    room.children_shapes.append(panel)

    specs = [
        ("objects-a", UnionType.UNION, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0),
        ("objects-b", UnionType.SUBTRACTION, (0.6, 0.4, 0.8), (0.0, 0.5, 0.0), 0.9),
        ("objects-c", UnionType.UNION, (-0.4, -0.3, 0.5), (0.2, -0.3, 0.1), 1.1),
    ]
    unions = [room]
    for ui, (name, ut, upos, urot, usc) in enumerate(specs):
        u = _union(name, ut, pos=upos, rot=urot, scale=usc)
        first = 0
        if ui == 0:
            for oname, sz, opos, orot in _OCTA:
                o = _shape(Shapes.OCTAHEDRON, pos=opos, rot=orot, size=(sz * 0.6,), name=oname)
                _mat(o, col=(0.0, 0.0, 0.0), spec=1.0, spec_col=(1.0, 1.0, 1.0), rough=0.555)
                u.children_shapes.append(o)
            first = 2
        for k in range(first, 7):
            kind = Shapes.SPHERE if rng.random() < 0.5 else Shapes.CUBE
            pos = (rng.uniform(-2.4, 2.4), rng.uniform(-1.2, 1.8), rng.uniform(-0.5, 4.0))
            rot = tuple(rng.uniform(-math.pi, math.pi, 3))
            if kind == Shapes.SPHERE:
                size = (rng.uniform(0.2, 0.75),)
            else:
                size = tuple(rng.uniform(0.2, 0.75, 3))
            # subtraction unions cut with their later members: keep those small
            if ut == UnionType.SUBTRACTION and k > 0:
                size = tuple(0.6 * v for v in size)
            aabb = not (ui == 2 and k in (5, 6))
            s = _shape(kind, pos=pos, rot=rot, size=size, aabb=aabb, name=f"{name}-{k}")
            col = tuple(rng.uniform(0.1, 0.95, 3))
            emissive = rng.random() < 0.12
            spec = float(rng.choice([0.0, 0.0, 0.3, 0.8]))
            _mat(s, col=col, brightness=3.0 if emissive else 0.0, spec=spec,
                 spec_col=tuple(rng.uniform(0.6, 1.0, 3)), rough=float(rng.uniform(0.0, 0.6)))
            u.children_shapes.append(s)
        unions.append(u)
    return SDFEditor(unions)


def nested_demo() -> SDFEditor:
    """Nested unions: exercises the compiler quirks of SURVEY.md A.9 (i)-(ii)
    (child-union results discarded by the index-0 assignment; map/bounds
    check[] index mismatch)."""
    outer = _union("outer", UnionType.UNION, pos=(0.1, 0.0, 0.3), rot=(0.0, 0.3, 0.0), scale=0.9)
    inner = _union("inner", UnionType.SUBTRACTION, pos=(0.3, 0.2, 0.0), scale=1.2)
    a = _shape(Shapes.CUBE, pos=(0.0, 0.0, 0.0), size=(0.6, 0.6, 0.6), rot=(0.4, 0.1, 0.2))
    _mat(a, col=(0.8, 0.3, 0.3))
    b = _shape(Shapes.SPHERE, pos=(0.2, 0.2, -0.2), size=(0.5,))
    _mat(b, col=(0.3, 0.8, 0.3))
    inner.children_shapes += [a, b]
    deeper = _union("deeper", UnionType.UNION, pos=(-0.5, 0.0, 0.0))
    c = _shape(Shapes.OCTAHEDRON, pos=(0.0, 0.5, 0.0), size=(0.5,), rot=(0.3, 0.2, 0.1))
    _mat(c, col=(0.3, 0.3, 0.9), spec=0.6, rough=0.2)
    deeper.children_shapes.append(c)
    inner.children_unions.append(deeper)
    outer.children_unions.append(inner)
    # emitters with aabb off: under quirk (ii) an aabb-guarded shape of a nested
    # graph reads a check[] entry bounds() never sets, and would stay dark
    d = _shape(Shapes.SPHERE, pos=(-0.9, -0.2, 0.4), size=(0.45,), aabb=False)
    _mat(d, col=(0.9, 0.9, 0.2), brightness=2.0)
    e = _shape(Shapes.CUBE, pos=(0.9, -0.4, 0.0), size=(0.3, 0.5, 0.3), aabb=False)
    _mat(e, col=(0.5, 0.5, 0.5), spec=0.4)
    outer.children_shapes += [d, e]
    top2 = _union("lamp")
    l = _shape(Shapes.SPHERE, pos=(0.0, 2.5, 0.0), size=(0.8,), aabb=False)
    _mat(l, brightness=3.0)
    top2.children_shapes.append(l)
    return SDFEditor([outer, top2])


def wide_graph(seed: int = 7, unions: int = 12, per_union: int = 8) -> SDFEditor:
    """c3's room plus `unions` x `per_union` small random shapes, all with
    AABBs: more than 64 check[] entries (exercises the high mask words)."""
    rng = np.random.default_rng(seed)
    ed = c3_graph32()
    for ui in range(unions):
        u = _union(f"cloud-{ui}", pos=(rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(0.0, 1.0)))
        for k in range(per_union):
            kind = Shapes.SPHERE if rng.random() < 0.6 else Shapes.CUBE
            size = (rng.uniform(0.05, 0.2),) if kind == Shapes.SPHERE else tuple(rng.uniform(0.05, 0.2, 3))
            s = _shape(kind, pos=(rng.uniform(-2.2, 2.2), rng.uniform(-1.0, 1.6), rng.uniform(0.0, 4.0)),
                       rot=tuple(rng.uniform(-1.0, 1.0, 3)), size=size, name=f"cloud-{ui}-{k}")
            _mat(s, col=tuple(rng.uniform(0.2, 0.9, 3)), brightness=2.0 if rng.random() < 0.1 else 0.0,
                 spec=float(rng.choice([0.0, 0.5])), rough=0.3)
            u.children_shapes.append(s)
        ed.header_unions.append(u)
    return ed


def cull_stress(seed: int = 11) -> SDFEditor:
    """c3's room plus clustered unions of every shape kind under scaled and
    rotated union/shape transforms: the distance-bound culling of the scene
    kernels drops shapes near its threshold.  Three unions
    carry values that switch the rule off (a negative cube size, a 1e-7 shape
    scale) or keep it on with a negative sphere radius."""
    rng = np.random.default_rng(seed)
    ed = c3_graph32()
    kinds = (Shapes.SPHERE, Shapes.CUBE, Shapes.TORUS, Shapes.OCTAHEDRON)
    for ui in range(6):
        u = _union(f"cluster-{ui}", pos=(rng.uniform(-1.2, 1.2), rng.uniform(-0.6, 0.9), rng.uniform(0.5, 3.0)),
                   rot=tuple(rng.uniform(-0.8, 0.8, 3)), scale=float(rng.uniform(0.6, 1.4)))
        for k in range(6):
            kind = kinds[(ui + k) % 4]
            if kind == Shapes.CUBE:
                size = tuple(rng.uniform(0.05, 0.3, 3))
            elif kind == Shapes.TORUS:
                size = (float(rng.uniform(0.1, 0.3)), float(rng.uniform(0.02, 0.1)))
            else:
                size = (float(rng.uniform(0.05, 0.3)),)
            sc = float(rng.uniform(0.5, 1.6))
            if ui == 3 and k == 2:
                size = (0.2, -0.1, 0.2)  # degenerate cube: no bound, the union's rule is off
                kind = Shapes.CUBE
            if ui == 4 and k == 4:
                sc = 1e-7  # 1/s beyond the bound's range: no bound, the union's rule is off
            if ui == 5 and k == 1:
                kind, size = Shapes.SPHERE, (-0.15,)  # negative radius: still bounded (R = r)
            s = _shape(kind, pos=tuple(rng.uniform(-0.5, 0.5, 3)), rot=tuple(rng.uniform(-math.pi, math.pi, 3)),
                       scale=sc, size=size, aabb=bool(rng.random() < 0.7), name=f"cluster-{ui}-{k}")
            _mat(s, col=tuple(rng.uniform(0.2, 0.9, 3)), brightness=2.0 if rng.random() < 0.15 else 0.0,
                 spec=float(rng.choice([0.0, 0.5])), rough=0.3)
            u.children_shapes.append(s)
        ed.header_unions.append(u)
    return ed


def tiny_union() -> SDFEditor:
    """Open space towards a distant backdrop, with two specks behind the
    camera: header unions of scale 1e-3 and 2e-3 whose shapes are ~1 unit in
    their own frame.  A union returns MAXHIT * s (= 10,
    20 world units) when none of its shapes combines, so rays through open
    space (parent distance > 10) check that the scene kernels' distance-bound
    culling of a union's first (assign) shape keeps the reference's value
    (containers.rs:244-252: u = shape overwrites MAXHIT)."""
    a = _union("anchor")
    lamp = _shape(Shapes.SPHERE, pos=(0.0, -0.2, 2.0), size=(0.6,), name="lamp")
    _mat(lamp, col=(0.9, 0.8, 0.7), brightness=2.0)
    box = _shape(Shapes.CUBE, pos=(1.2, 0.4, 3.0), rot=(0.3, 0.5, 0.0), size=(0.3, 0.3, 0.3), name="box")
    _mat(box, col=(0.3, 0.6, 0.9), spec=0.5, rough=0.2)
    wall = _shape(Shapes.CUBE, pos=(0.0, 0.0, 40.0), size=(80.0, 80.0, 1.0), aabb=False, name="backdrop")
    _mat(wall, col=(0.7, 0.7, 0.7), brightness=0.5)
    a.children_shapes += [lamp, box, wall]
    # behind the camera: farther than the running distance while rays cross
    # the open space towards the backdrop, so their shapes are dropped
    sp = _union("speck-a", pos=(0.4, 0.3, -20.0), rot=(0.2, 0.1, 0.4), scale=1e-3)
    for k, (kind, pos, size, aabb) in enumerate([(Shapes.SPHERE, (0, 0, 0), (1.0,), False),
                                                 (Shapes.CUBE, (1.5, 0, 0), (0.8, 0.8, 0.8), False),
                                                 (Shapes.SPHERE, (0, 1.5, 0), (0.5,), True)]):
        s = _shape(kind, pos=pos, size=size, aabb=aabb, name=f"speck-a-{k}")
        _mat(s, col=(0.8, 0.2, 0.2), brightness=5.0)
        sp.children_shapes.append(s)
    sb = _union("speck-b", pos=(-0.5, 0.2, -25.0), scale=2e-3)
    s = _shape(Shapes.CUBE, size=(1.0, 1.0, 1.0), aabb=False, name="speck-b-0")
    _mat(s, col=(0.2, 0.8, 0.2))
    sb.children_shapes.append(s)
    return SDFEditor([a, sp, sb])


def far_box() -> SDFEditor:
    """c2 plus a sphere 1e20 units away with its AABB on: one box coordinate
    outside the reciprocal-division guard, so every ray of
    the scene takes bounds()'s IEEE-division path (scene kernels: the baked
    'false' branch and the table kernel's fast_bounds = 0)."""
    ed = c2_sphere_box_torus()
    u = _union("far")
    s = _shape(Shapes.SPHERE, pos=(1e20, 0.0, 0.0), size=(1.0,), name="far")
    _mat(s, col=(0.5, 0.5, 0.5))
    u.children_shapes.append(s)
    ed.header_unions.append(u)
    return ed


_DEPRECATED_KINDS = {"Sphere": Shapes.SPHERE, "Cube": Shapes.CUBE, "OctahedronExact": Shapes.OCTAHEDRON}


def deprecated_map(nodes) -> SDFEditor:
    """A map saved by the reference's deprecated node editor
    (assets/maps/*.json: a list of serde `Node`s,
    assets/depricated/node_editor_package.rs:204-218 + its `Material`) as
    a current editor scene.  One header union holds the nodes in file order.
    Each node keeps its shape (OctahedronExact -> Octahedron), scale, size,
    position and rotation.  Material fields are copied one for one
    (light_strength -> Brightness).  A light colour of (0, 0, 0) becomes
    the live editor's default (1, 1, 1): the current Mat normalises the
    light colour, and zero would make every hit NaN.  AABB culling is on,
    with the editor's default exaggeration.  `nodes`: the parsed JSON list,
    or a path to the file."""
    if isinstance(nodes, str):
        import json

        with open(nodes) as f:
            nodes = json.load(f)
    u = _union("map")
    for n in nodes:
        kind = _DEPRECATED_KINDS[n["shape"]]
        m = n["material"]
        light = tuple(m["light"])
        s = _shape(kind, pos=tuple(n["position"]), rot=tuple(n["rotation"]), scale=n["scale"],
                   size=tuple(n["size"]), name=n["title"])
        _mat(s, col=tuple(m["color"]), brightness=m["light_strength"],
             light=light if any(v != 0.0 for v in light) else (1.0, 1.0, 1.0), spec=m["spec"],
             spec_col=tuple(m["spec_col"]), rough=m["roughness"])
        mat = s.material
        mat.ior.set(m["ior"])
        mat.refract_chance.set(m["refraction_chance"])
        mat.refract_roughness.set(m["refraction_roughness"])
        mat.refract_color.set(tuple(m["refraction_color"]))
        u.children_shapes.append(s)
    return SDFEditor([u])


def c3_no_aabb() -> SDFEditor:
    """c3 with every Transform.aabb off (profiling aid: no per-lane culling)."""
    ed = c3_graph32()
    for u in ed.header_unions:
        for sh in u.children_shapes:
            sh.transform.aabb = False
    return ed


def nan_cube(which: str = "position") -> SDFEditor:
    """An emissive octahedron in front of a cube whose transform holds a NaN:
    its position x ("position"), its rotation about x ("rotation": 2e7 is
    beyond the range of the reference's sin / cos), or its
    union's rotation about z with none of its own ("union-rotation").  The
    reference multiplies by full rotation matrices, and 0 * NaN = NaN makes
    all three of the cube's coordinates NaN; sdCube's min / max drop NaNs, so
    its distance is 0 everywhere and every ray ends on it at once.  Kernels
    that skip the matrices' zero terms keep a finite coordinate and see a slab
    instead (found by random value edits on fuzz_scene(24); pt_derive.cpp
    makes such a node's whole translation NaN)."""
    a = _union("front", scale=2.0, pos=(0.0, 0.06, 0.07))
    o = _shape(Shapes.OCTAHEDRON, pos=(-0.37, -0.65, 0.0), rot=(1.36, 1.46, -2.63), scale=0.64, size=(0.83,),
               aabb=False, name="octahedron")
    _mat(o, col=(0.72, 0.26, 0.28), brightness=1.6, spec=1.0, spec_col=(0.7, 0.68, 0.92), rough=0.3)
    a.children_shapes.append(o)
    b = _union("behind", pos=(0.19, 0.23, 0.47), rot=(-0.46, 0.0, 2e7 if which == "union-rotation" else 0.0))
    nan = float("nan")
    c = _shape(Shapes.CUBE, pos=(nan if which == "position" else 0.4, 0.8, 0.0),
               rot={"rotation": (2e7, 0.0, 0.0), "union-rotation": (0.0, 0.0, 0.0)}.get(which, (-3.03, 0.0, 2.02)),
               size=(0.61, 0.67, 0.65), aabb=False,
               name="cube")
    _mat(c, col=(0.59, 0.65, 0.91), brightness=3.8, light=(0.2, 0.5, 1.0), spec=0.35, rough=0.2)
    b.children_shapes.append(c)
    return SDFEditor([a, b])


def nan_cube_rotation() -> SDFEditor:
    return nan_cube("rotation")


def nan_cube_union_rotation() -> SDFEditor:
    return nan_cube("union-rotation")


_FUZZ_KINDS = (Shapes.SPHERE, Shapes.CUBE, Shapes.TORUS, Shapes.OCTAHEDRON)
FUZZ_DEEP_LEVELS = 8  # the interpreter's union stack (pt_device.h PT_MAX_DEPTH)


def _fuzz_scale(rng, outside: bool) -> float:
    """A scale: exactly 1 (p 0.4), the dyadic 0.5 or 2 (0.1 each), a
    non-dyadic one in [0.6, 1.6] (0.25), and for unions (`outside`) 0.4 or 2.5
    (0.15 together, 1/s outside [1/2, 2]; shapes get more non-dyadic ones)."""
    r = rng.random()
    if r < 0.4:
        return 1.0
    if r < 0.5:
        return 0.5
    if r < 0.6:
        return 2.0
    if r < 0.85 or not outside:
        return float(rng.uniform(0.6, 1.6))
    return 0.4 if rng.random() < 0.5 else 2.5


def _fuzz_vec(rng, lo, hi, p_all: float, p_one: float):
    """Three components from [lo[k], hi[k]]; all exactly 0 with p_all, else
    each exactly 0 with p_one."""
    v = [float(rng.uniform(lo[k], hi[k])) for k in range(3)]
    zero_all = rng.random() < p_all
    return tuple(0.0 if zero_all or rng.random() < p_one else x for x in v)


def _fuzz_shape(rng, name: str, world: float, small: bool) -> Shape:
    """One shape of about 0.5-1.8 world units (`world`: its ancestors' scale
    product), or with p 0.2 a cube slab whose middle half-extent is 1.5-4 world
    units (the scene kernels' one-face cube path); `small`: 0.6 of that, for
    the later members of a Subtraction union."""
    kind = _FUZZ_KINDS[int(rng.integers(4))]
    sc = _fuzz_scale(rng, outside=False)
    k = (0.6 if small else 1.0) / (sc * world)
    if kind == Shapes.CUBE:
        if rng.random() < 0.2:
            size = [float(rng.uniform(1.5, 4.0)) / (sc * world), float(rng.uniform(1.5, 4.0)) / (sc * world),
                    float(rng.uniform(0.1, 0.5)) / (sc * world)]
            size = tuple(size[j] for j in rng.permutation(3))
        else:
            size = tuple(float(v) * k for v in rng.uniform(0.5, 1.6, 3))
    elif kind == Shapes.TORUS:
        size = (float(rng.uniform(0.9, 1.6)) * k, float(rng.uniform(0.25, 0.5)) * k)
    else:
        size = (float(rng.uniform(0.7, 1.8)) * k,)
    pos = _fuzz_vec(rng, (-3.0 / world, -2.0 / world, -0.5 / world), (3.0 / world, 2.0 / world, 3.5 / world), 0.2, 0.15)
    rot = _fuzz_vec(rng, (-math.pi,) * 3, (math.pi,) * 3, 0.2, 0.3)
    s = _shape(kind, pos=pos, rot=rot, scale=sc, size=size, aabb=bool(rng.random() < 0.7), name=name,
               ex=(1.0, 1.3, 2.0)[int(rng.integers(3))])
    spec = (0.0, 0.0, float(rng.uniform(0.1, 0.9)), 1.0)[int(rng.integers(4))]
    _mat(s, col=tuple(rng.uniform(0.1, 0.95, 3)), brightness=float(rng.uniform(1.5, 4.0)) if rng.random() < 0.35 else 0.0,
         light=(1.0, 1.0, 1.0) if rng.random() < 0.5 else tuple(rng.uniform(0.3, 1.0, 3)), spec=spec,
         spec_col=tuple(rng.uniform(0.6, 1.0, 3)), rough=float(rng.uniform(0.0, 0.6)))
    return s


def _fuzz_union(rng, name: str, depth: int, world: float, budget: list) -> Union:
    """One union at nesting `depth` (1: a header union) with 0-2 child unions
    down to depth 4 and 0-4 shapes; `budget[0]` caps the nodes still to make."""
    ut = UnionType.SUBTRACTION if rng.random() < 0.3 else UnionType.UNION
    sc = _fuzz_scale(rng, outside=True)
    u = _union(name, ut, pos=_fuzz_vec(rng, (-0.5 / world,) * 3, (0.5 / world,) * 3, 0.35, 0.2),
               rot=_fuzz_vec(rng, (-0.6,) * 3, (0.6,) * 3, 0.5, 0.3), scale=sc)
    budget[0] -= 1
    n_child = (0, 0, 0, 1, 1, 2)[int(rng.integers(6))] if depth < 4 else 0
    n_shape = (0, 1, 2, 2, 3, 4)[int(rng.integers(6))]
    for k in range(n_child):
        if budget[0] > 0:
            u.children_unions.append(_fuzz_union(rng, f"{name}.{k}", depth + 1, world * sc, budget))
    for k in range(n_shape):
        if budget[0] > 0:
            budget[0] -= 1
            u.children_shapes.append(_fuzz_shape(rng, f"{name}-{k}", world * sc,
                                                 small=ut == UnionType.SUBTRACTION and k > 0))
    return u


def fuzz_scene(seed: int, profile: str = "mixed") -> SDFEditor:
    """A random editor tree, the same for the same (seed, profile): values come
    from np.random.default_rng(seed) only (the Floats' slot hashes are fresh
    each time, as for every scene here, and reach no value).

    profile "mixed": 1-5 header unions and at most 30 nodes (unions + shapes);
    seeds whose draw stays at 12 program ops or fewer (a union counts two)
    are the ones cheap enough to compile as scene kernels.  The distributions, per node:

    * unions: Subtraction with p 0.3; 0-2 child unions (p 1/2, 1/3, 1/6) down to
      nesting depth 4, and 0-4 shapes (p 1/6 for 0), so empty unions, unions
      with only child unions (whose result survives) and unions whose first
      shape overwrites their child unions all occur;
    * shapes: the four kinds with equal chance, so each occurs as the first
      (assign) member, as a later member of a Union and of a Subtraction union;
    * scale: exactly 1 (p 0.4), 0.5, 2 (0.1 each), non-dyadic in [0.6, 1.6];
      unions also 0.4 and 2.5 (p 0.15), outside [1/2, 2];
    * position: all three components exactly 0 with p 0.2 (shapes) / 0.35
      (unions), else each exactly 0 with p 0.15 / 0.2;
    * rotation: all exactly 0 with p 0.2 (shapes) / 0.5 (unions), else each
      exactly 0 with p 0.3 -- every PT_NF_* identity flag is set in some node
      and clear in some;
    * boxes: on with p 0.7, exaggeration 1.0, 1.3 or 2.0;
    * cubes: half-extents of 0.5-1.6 world units, or (p 0.2) a slab with a
      middle half-extent of 1.5-4 world units: both sides of fast_cube's threshold;
    * materials: emitters with p 0.35 (brightness 1.5-4, light colour white or
      random), and one direct shape of a header union is always an emitter
      without a box (a lamp union is added when no header union has a shape),
      so the image is lit;
      specular chance 0 (p 1/2), fractional, or 1.

    profile "deep": one chain of unions nested exactly FUZZ_DEEP_LEVELS deep,
    one shape at every level, the same per-node distributions."""
    rng = np.random.default_rng(seed)
    if profile == "deep":
        top, world, parent = None, 1.0, None
        for d in range(FUZZ_DEEP_LEVELS):
            budget = [1]
            u = _fuzz_union(rng, f"deep-{d}", FUZZ_DEEP_LEVELS, world, budget)  # (transform and type only)
            u.children_unions, u.children_shapes = [], [_fuzz_shape(rng, f"deep-{d}-0", world * u.transform.scale.val,
                                                                    small=False)]
            world *= u.transform.scale.val
            if parent is None:
                top = u
            else:
                parent.children_unions.append(u)
            parent = u
        unions = [top]
    elif profile == "mixed":
        budget = [30]
        unions = []
        for k in range(int(rng.integers(1, 6))):
            if budget[0] > 0:
                unions.append(_fuzz_union(rng, f"u{k}", 1, 1.0, budget))
    else:
        raise ValueError(f"unknown fuzz profile {profile!r}")
    direct = [s for u in unions for s in u.children_shapes]
    if not direct:
        lamp = _union("lamp")
        lamp.children_shapes.append(_shape(Shapes.SPHERE, pos=(float(rng.uniform(-1.0, 1.0)), 2.0, 1.0), size=(0.8,),
                                           aabb=False, name="lamp"))
        unions.append(lamp)
        direct = lamp.children_shapes
    lamp = direct[int(rng.integers(len(direct)))]
    lamp.material.brightness.set(float(rng.uniform(1.5, 4.0)))
    lamp.transform.aabb = False  # (a boxed shape of a nested graph can read a check[] entry bounds() never sets, and go dark)
    return SDFEditor(unions)


# Seeds of fuzz_scene(seed) for the interpreter kernels.  Chosen from 0..199:
# every one renders a lit image (tests/test_scene_fuzz.py), and together they
# hold every feature of fuzz_scene's docstring (the census there).
FUZZ_SEEDS = (0, 2, 4, 5, 7, 8, 13, 17, 19, 20, 22, 23, 24, 28, 30, 31, 34, 35, 40, 41, 44, 45, 48, 49, 50, 51, 52, 53, 56, 58,
              62, 64, 65, 66, 67, 70, 71, 73, 74, 75, 78, 84, 85, 86, 87, 88, 89, 93)
# (seed, profile) of the scenes small enough to compile as scene kernels (at
# most 12 program ops, a union counting two; the deep chain needs 24 by
# construction): registered below as
# "fuzz-<seed>", and build.py ships their kernels in lib/jitcache.
FUZZ_JIT_SEEDS = ((56, "mixed"), (154, "mixed"), (259, "mixed"), (3521, "mixed"), (15793, "mixed"), (2, "deep"))


def _fuzz_maker(seed: int, profile: str):
    def make() -> SDFEditor:
        return fuzz_scene(seed, profile)

    make.__name__ = f"fuzz_scene_{seed}_{profile}"
    return make


SCENES = {
    "empty": empty,
    "c1": c1_default,
    "c2": c2_sphere_box_torus,
    "c3": c3_graph32,
    "nested": nested_demo,
    "c3_noaabb": c3_no_aabb,
    "wide": wide_graph,
    "cull": cull_stress,
    "tiny": tiny_union,
    "farbox": far_box,
    "nan-position": nan_cube,
    "nan-rotation": nan_cube_rotation,
    "nan-union-rotation": nan_cube_union_rotation,
}
SCENES.update({f"fuzz-{seed}": _fuzz_maker(seed, profile) for seed, profile in FUZZ_JIT_SEEDS})

# BASELINE.json configs -> (scene, width, height, spp, bounces)
CONFIGS = {
    "c1": ("c1", 256, 256, 1, 1),
    "c2": ("c2", 1920, 1080, 64, 4),
    "c3": ("c3", 1920, 1080, 256, 8),
    "c4": ("c3", 3840, 2160, 256, 8),
    "c5": ("c3", 1920, 1080, 1024, 16),
}
