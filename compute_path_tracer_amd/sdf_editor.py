"""Host mirror of the reference's SDF editor node graph and its compiler.

Mirrors ``src/sdf_editor`` of zachdedoo13/compute_path_tracer (snapshot
2024-10-08): the same node types (``Union``, ``Shape``, ``Transform``,
``Material``, ``Float``, ``V3``), the same defaults, the same serde JSON
layout for save/load (``sdf_editor.rs:131-167``) and the same compile/update
split (``RecUpdate``, ``primitives.rs:160-190``).  What changes is the compile
target: instead of GLSL text spliced into the compute shader
(``SDFEditor::compile``, ``sdf_editor.rs:186-246``) the tree is compiled by the
native ``pt_compile_scene`` into an op list + ``data[]`` with the reference's
exact slot numbering, which :class:`compute_path_tracer_amd.path_tracer.PathTracer`
uploads through the C ABI.  The egui UI code is out of scope.
"""
from __future__ import annotations

import ctypes
import json
import secrets
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _native as N

F32_MAX = float(np.finfo(np.float32).max)

# speeds, primitives.rs:193-196
S1 = 0.001
S2 = 0.01
S3 = 0.1


def gen_hash() -> int:
    """primitives.rs:12-17: a random u128 identifying a Float's data[] slot."""
    return secrets.randbits(128) ^ secrets.randbits(128)


class Float:
    """primitives.rs:203-267."""

    def __init__(self, name: str, speed: float, val: float, rng: Tuple[float, float] = (-F32_MAX, F32_MAX),
                 hash_: Optional[int] = None):
        self.val = float(np.float32(val))
        self.range = (float(rng[0]), float(rng[1]))
        self.speed = float(speed)
        self.name = name
        self.hash = gen_hash() if hash_ is None else int(hash_)

    @classmethod
    def new(cls, name, speed, val, rng):
        return cls(name, speed, val, rng)

    @classmethod
    def inv(cls, name, speed, val):
        return cls(name, speed, val, (-F32_MAX, F32_MAX))

    @classmethod
    def percent(cls, name, speed, val):
        return cls(name, speed, val, (0.0, 1.0))

    def set(self, v: float) -> None:
        lo, hi = self.range
        self.val = float(np.float32(min(max(v, lo), hi)))

    def compile(self, comp_data: "CompData") -> int:
        return comp_data.data_array.get_index(self.val, self.hash)

    def refresh(self, comp_data: "CompData") -> None:
        comp_data.data_array.refresh(self.hash, self.val)

    def rehash(self) -> None:
        self.hash = gen_hash()

    def to_json(self):
        return {"val": self.val, "range": {"start": self.range[0], "end": self.range[1]}, "speed": self.speed,
                "name": self.name, "hash": self.hash}

    @classmethod
    def from_json(cls, d):
        r = d.get("range", {"start": -F32_MAX, "end": F32_MAX})
        return cls(d["name"], d["speed"], d["val"], (r["start"], r["end"]), d["hash"])

    def floats(self):
        yield self


class Node:
    """A serde struct of the editor.  ``FIELDS`` states its members once, as
    (name, kind) in the key order of its ``to_json``: kind is Float or a Node
    class (saved through its own to_json / from_json), ``[kind]`` for a list
    of them, ``None`` for a plain value or a cast such as ``bool``.  FIELDS
    names every attribute, so ``from_json`` fills a bare instance.  ``COMPILE``
    names the members that hold Floats in the order the reference's compile
    visits them (what ``floats()`` yields) and ``REFRESH`` in the order its
    refresh does (default: COMPILE); the three orders differ.  Float (the
    leaf) and Shapes (a serde enum) write their own by hand."""

    FIELDS: Tuple = ()
    COMPILE: Tuple[str, ...] = ()
    REFRESH: Optional[Tuple[str, ...]] = None

    def floats(self):
        for name in self.COMPILE:
            yield from getattr(self, name).floats()

    def rehash(self):
        for f in self.floats():
            f.rehash()

    def refresh(self, comp_data):
        for name in self.COMPILE if self.REFRESH is None else self.REFRESH:
            member = getattr(self, name)
            for m in member if isinstance(member, list) else (member,):
                m.refresh(comp_data)

    def to_json(self):
        def save(v):
            return [save(x) for x in v] if isinstance(v, list) else v.to_json() if hasattr(v, "to_json") else v

        return {name: save(getattr(self, name)) for name, _ in self.FIELDS}

    @classmethod
    def from_json(cls, d):
        def load(kind, v):
            if isinstance(kind, list):
                return [load(kind[0], x) for x in v]
            return v if kind is None else kind.from_json(v) if hasattr(kind, "from_json") else kind(v)

        node = cls.__new__(cls)
        for name, kind in cls.FIELDS:
            setattr(node, name, load(kind, d[name]))
        return node


class V3(Node):
    """primitives.rs:269-331."""

    FIELDS = (("x", Float), ("y", Float), ("z", Float), ("name", None))
    COMPILE = ("x", "y", "z")

    def __init__(self, x: Float, y: Float, z: Float, name: str):
        self.x, self.y, self.z, self.name = x, y, z, name

    @classmethod
    def xyz(cls, name, speed, val):
        return cls(Float.inv("X", speed, val), Float.inv("Y", speed, val), Float.inv("Z", speed, val), name)

    @classmethod
    def rgb(cls, name):
        return cls(Float.inv("R", 1.0, 1.0), Float.inv("G", 1.0, 1.0), Float.inv("B", 1.0, 1.0), name)

    def vals(self) -> List[float]:
        return [self.x.val, self.y.val, self.z.val]

    def set(self, v) -> None:
        self.x.set(v[0]); self.y.set(v[1]); self.z.set(v[2])


class Transform(Node):
    """data_structures.rs:10-111."""

    FIELDS = (("position", V3), ("rotation", V3), ("scale", Float), ("aabb_exaggeration", Float), ("aabb", bool))
    COMPILE = ("scale", "position", "rotation", "aabb_exaggeration")  # Transform::compile
    # data_structures.rs:98-103 (with shared hashes the last write wins, so the order matters)
    REFRESH = ("position", "rotation", "scale", "aabb_exaggeration")

    def __init__(self):
        self.position = V3.xyz("Position", S2, 0.0)
        self.rotation = V3.xyz("Rotation", S1, 0.0)
        self.scale = Float.new("Scale", S1, 1.0, (0.0, F32_MAX))
        self.aabb_exaggeration = Float.new("AABB_exaggeration", S2, 1.3, (0.0, 10.0))
        self.aabb = True


class Material(Node):
    """data_structures.rs:115-221 (Mat order of test_compute.glsl:45-59)."""

    FIELDS = (("color", V3), ("brightness", Float), ("light_col", V3), ("specular_chance", Float),
              ("specular_color", V3), ("roughness", Float), ("ior", Float), ("refract_chance", Float),
              ("refract_roughness", Float), ("refract_color", V3))
    COMPILE = tuple(name for name, _ in FIELDS)

    def __init__(self):
        self.color = V3.rgb("Surface Color")
        self.brightness = Float.new("Brightness", S2, 0.0, (0.0, F32_MAX))
        self.light_col = V3.rgb("Light Color")
        self.specular_chance = Float.percent("Spec chance", S1, 0.0)
        self.specular_color = V3.rgb("Spec color")
        self.roughness = Float.new("Roughness", S1, 0.0, (0.0, F32_MAX))
        self.ior = Float.inv("IOR", S1, 0.0)
        self.refract_chance = Float.percent("Refract chance", S1, 0.0)
        self.refract_roughness = Float.inv("Refract roughness", S1, 0.0)
        self.refract_color = V3.rgb("Refract color")

    def values(self) -> List[float]:
        return [f.val for f in self.floats()]


MATERIAL_FIELDS = Material.COMPILE


class Shapes(Node):
    """containers.rs:259-319 (Sphere, Cube, Plane) + Torus/Octahedron
    extensions.  A serde enum, not a struct: its Floats are the ``params``
    list and its to_json / from_json write the enum forms out by hand."""

    SPHERE, CUBE, PLANE, TORUS, OCTAHEDRON = "Sphere", "Cube", "Plane", "Torus", "Octahedron"
    KIND = {SPHERE: N.PT_NODE_SPHERE, CUBE: N.PT_NODE_CUBE, PLANE: N.PT_NODE_PLANE, TORUS: N.PT_NODE_TORUS,
            OCTAHEDRON: N.PT_NODE_OCTAHEDRON}

    def __init__(self, kind: str = SPHERE, params: Optional[List[Float]] = None):
        self.kind = kind
        if params is None:
            if kind == self.SPHERE:
                params = [Float.inv("Size", S2, 1.0)]
            elif kind == self.CUBE:
                params = list(V3.xyz("Size", S2, 1.0).floats())
            elif kind == self.TORUS:
                params = [Float.inv("Major radius", S2, 1.0), Float.inv("Minor radius", S2, 0.25)]
            elif kind == self.OCTAHEDRON:
                params = [Float.inv("Size", S2, 1.0)]
            else:
                params = []
        self.params = params

    def floats(self):
        yield from self.params

    def refresh(self, comp_data):
        for f in self.params:
            f.refresh(comp_data)

    def to_json(self):
        if self.kind == self.PLANE:
            return "Plane"
        if self.kind == self.CUBE:
            return {"Cube": V3(*self.params, "Size").to_json()}
        if self.kind == self.TORUS:
            return {"Torus": [p.to_json() for p in self.params]}
        return {self.kind: self.params[0].to_json()}

    @classmethod
    def from_json(cls, d):
        if d == "Plane":
            return cls(cls.PLANE, [])
        (kind, v), = d.items()
        if kind == cls.CUBE:
            return cls(kind, list(V3.from_json(v).floats()))
        if kind == cls.TORUS:
            return cls(kind, [Float.from_json(p) for p in v])
        return cls(kind, [Float.from_json(v)])


class Shape(Node):
    """containers.rs:322-476."""

    FIELDS = (("transform", Transform), ("material", Material), ("current_shape", Shapes), ("name", None))
    COMPILE = ("transform", "current_shape", "material")  # Shape::compile: transform, shape settings, material
    REFRESH = ("transform", "material", "current_shape")  # containers.rs:466-470: the shape's size last

    def __init__(self, kind: str = Shapes.SPHERE):
        self.transform = Transform()
        self.material = Material()
        self.current_shape = Shapes(kind)
        self.name = "Shape"


class UnionType:
    UNION = "Union"
    SUBTRACTION = "Subtraction"


class Union(Node):
    """containers.rs:8-203."""

    COMPILE = ("transform",)  # (the union's own Floats; its children are nodes of their own)
    REFRESH = ("transform", "children_shapes", "children_unions")  # containers.rs:204-212

    def __init__(self, union_type: str = UnionType.UNION):
        self.name = "Union"
        self.transform = Transform()
        self.union_type = union_type
        self.children_unions: List[Union] = []
        self.children_shapes: List[Shape] = []


Union.FIELDS = (("name", None), ("transform", Transform), ("union_type", None), ("children_unions", [Union]),
                ("children_shapes", [Shape]))  # (after the class: it names itself)


class DataArray:
    """primitives.rs:59-157 without the wgpu buffer (the C ABI owns the device copy)."""

    def __init__(self):
        self.data: List[float] = [6969.69]
        self.seen: Dict[int, int] = {}

    def get_index(self, val: float, hash_: int) -> int:
        if hash_ in self.seen:
            return self.seen[hash_]
        self.data.append(float(np.float32(val)))
        self.seen[hash_] = len(self.data) - 1
        return self.seen[hash_]

    def refresh(self, hash_: int, val: float) -> None:
        if hash_ not in self.seen:
            raise KeyError("Float hash not compiled (primitives.rs:154 panics here)")
        self.data[self.seen[hash_]] = float(np.float32(val))

    def as_array(self) -> np.ndarray:
        return np.asarray(self.data, dtype=np.float32)


class RecUpdate:
    """primitives.rs:160-190."""

    def __init__(self, compile_: bool = True, update: bool = True):
        self.queue_compile = compile_
        self.queue_update = update

    def reset(self):
        self.queue_compile = self.queue_update = False

    def update(self):
        self.queue_update = True

    def compile(self):
        self.queue_compile = True

    def both(self):
        self.queue_compile = self.queue_update = True


class CompData:
    """primitives.rs:21-57."""

    def __init__(self):
        self.data_array = DataArray()
        self.rec_update = RecUpdate(True, True)
        self.aabb_index = 0

    def reset_data_array(self):
        self.data_array.data = [6969.69]
        self.data_array.seen.clear()


@dataclass
class Program:
    """What SDFEditor::compile now produces: the map()/bounds() program."""

    ops: ctypes.Array
    aabbs: ctypes.Array
    n_ops: int
    n_aabb: int
    n_check: int
    data: np.ndarray = field(default_factory=lambda: np.zeros(1, np.float32))

    def op_dicts(self) -> List[dict]:
        return [struct_dict(self.ops[i]) for i in range(self.n_ops)]

    def aabb_dicts(self) -> List[dict]:
        return [struct_dict(self.aabbs[i]) for i in range(self.n_aabb)]


def struct_dict(s: ctypes.Structure) -> dict:
    """A ctypes structure as a dict in ``_fields_`` order: scalars as ints, arrays as lists."""
    return {name: list(getattr(s, name)) if issubclass(t, ctypes.Array) else getattr(s, name)
            for name, t in s._fields_}


def key_floats(node) -> List[Optional[Float]]:
    """A Union's or Shape's Floats in pt_float_key order (PT_NODE_FLOATS):
    scale, position xyz, rotation xyz, exaggeration, size[3], material[18];
    None where the node has no such Float (a union has the first 8)."""
    size = list(node.current_shape.floats()) if isinstance(node, Shape) else []
    material = list(node.material.floats()) if isinstance(node, Shape) else [None] * 18
    return [*node.transform.floats(), *size, *[None] * (3 - len(size)), *material]


def node_keys(node) -> List[int]:
    """The node's Float hashes in pt_float_key order; 0 where it has no such Float."""
    return [0 if f is None else f.hash for f in key_floats(node)]


def node_row(node, parent: int) -> dict:
    """One row of ``flatten``: the pt_scene_node of a Union or Shape, its
    values in key_floats order (0 where it has no such Float), and its keys."""
    v = [0.0 if f is None else f.val for f in key_floats(node)]
    is_union = isinstance(node, Union)
    return {"kind": N.PT_NODE_UNION if is_union else Shapes.KIND[node.current_shape.kind], "parent": parent,
            "union_type": N.PT_UNION_TYPE_SUBTRACTION if is_union and node.union_type == UnionType.SUBTRACTION
            else N.PT_UNION_TYPE_UNION, "aabb": int(node.transform.aabb), "scale": v[0], "position": v[1:4],
            "rotation": v[4:7], "aabb_exaggeration": v[7], "size": v[8:11], "material": v[11:],
            "keys": node_keys(node)}


def keys_to_ctypes(rows: List[dict]):
    """Rows' "keys" as a pt_float_key array (None when no row carries keys)."""
    if not any(r.get("keys") for r in rows):
        return None
    arr = (N.FloatKey * (max(1, len(rows)) * N.PT_NODE_FLOATS))()
    for i, r in enumerate(rows):
        for k, h in enumerate(r.get("keys") or []):
            arr[i * N.PT_NODE_FLOATS + k].lo = h & 0xFFFFFFFFFFFFFFFF
            arr[i * N.PT_NODE_FLOATS + k].hi = (h >> 64) & 0xFFFFFFFFFFFFFFFF
    return arr


def flatten(header_unions: List[Union]) -> Tuple[List[dict], List[object]]:
    """Pre-order flattening: each node's parent precedes it; a union's child
    unions precede its shapes (the order Union::compile visits them)."""
    rows: List[dict] = []
    objs: List[object] = []

    def visit(u: Union, parent: int):
        idx = len(rows)
        rows.append(node_row(u, parent))
        objs.append(u)
        for c in u.children_unions:
            visit(c, idx)
        for s in u.children_shapes:
            rows.append(node_row(s, idx))
            objs.append(s)

    for u in header_unions:
        visit(u, -1)
    return rows, objs


def nodes_to_ctypes(rows: List[dict]) -> ctypes.Array:
    arr = (N.SceneNode * max(1, len(rows)))()
    for i, r in enumerate(rows):
        for name, t in N.SceneNode._fields_:
            setattr(arr[i], name, t(*r[name]) if issubclass(t, ctypes.Array) else r[name])
    return arr


def compile_rows(rows: List[dict]) -> Program:
    """Native pt_compile_scene_keyed on flattened rows (two-call pattern):
    Floats sharing a hash share a data[] slot (DataArray::get_index)."""
    L = N.lib()
    nodes = nodes_to_ctypes(rows)
    keys = keys_to_ctypes(rows)
    n_ops, n_aabb, n_data, n_check = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    rc = L.pt_compile_scene_keyed(nodes, len(rows), keys, None, 0, ctypes.byref(n_ops), None, 0, ctypes.byref(n_aabb),
                                  None, 0, ctypes.byref(n_data), ctypes.byref(n_check))
    N.check("pt_compile_scene_keyed", rc)
    ops = (N.Op * max(1, n_ops.value))()
    aabbs = (N.Aabb * max(1, n_aabb.value))()
    data = np.zeros(n_data.value, dtype=np.float32)
    rc = L.pt_compile_scene_keyed(nodes, len(rows), keys, ops, n_ops.value, ctypes.byref(n_ops), aabbs, n_aabb.value,
                                  ctypes.byref(n_aabb), N.fptr(data), n_data.value, ctypes.byref(n_data),
                                  ctypes.byref(n_check))
    N.check("pt_compile_scene_keyed", rc)
    return Program(ops, aabbs, n_ops.value, n_aabb.value, n_check.value, data)


class SDFEditor:
    """sdf_editor.rs:13-253: the tree, its JSON save/load and its compiler."""

    def __init__(self, header_unions: Optional[List[Union]] = None):
        if header_unions is None:  # SDFEditor::new, sdf_editor.rs:20-33
            header_unions = [Union()]
            header_unions[0].children_shapes.append(Shape())
        self.header_unions = header_unions
        self.save_name = ""

    # -- compiler ---------------------------------------------------------
    def compile(self, comp_data: CompData) -> Program:
        """SDFEditor::compile: reset data[], allocate slots, emit the program.

        The slot of every Float is registered in comp_data.data_array.seen so
        later value edits go through refresh without a recompile."""
        comp_data.reset_data_array()
        rows, objs = flatten(self.header_unions)
        prog = compile_rows(rows)
        # register Float -> slot exactly as Float::compile would have
        ops = prog.op_dicts()
        shape_ops = [o for o in ops if o["opcode"] == N.PT_OP_SHAPE]
        union_ops = [o for o in ops if o["opcode"] == N.PT_OP_UNION_BEGIN]
        next_op = {Shape: iter(shape_ops), Union: iter(union_ops)}
        data = comp_data.data_array
        data.data = [float(x) for x in prog.data]
        for obj in objs:
            op = next(next_op[type(obj)])
            slots = [op["scale"], *op["position"], *op["rotation"], op["aabb_exaggeration"], *op["size"],
                     *op["material"]]  # (pt_op's operands are in pt_float_key order)
            for f, slot in zip(key_floats(obj), slots):
                if f is not None:
                    data.seen[f.hash] = slot
        comp_data.aabb_index = prog.n_check if prog.n_check > 1 or shape_ops else 0
        return prog

    def data_update(self, comp_data: CompData) -> None:
        """sdf_editor.rs:248-252: value-only refresh of data[]."""
        for u in self.header_unions:
            u.refresh(comp_data)

    def update(self, path_tracer, comp_data: CompData) -> None:
        """SDFEditor::update (sdf_editor.rs:35-47) + SDFEditorPackage::update (:272-283)."""
        changed = comp_data.rec_update.queue_compile or comp_data.rec_update.queue_update
        if comp_data.rec_update.queue_compile:
            prog = self.compile(comp_data)
            path_tracer.remake_pipeline(prog)
        if comp_data.rec_update.queue_update:
            self.data_update(comp_data)
        comp_data.rec_update.reset()
        if changed:
            path_tracer.changed = True
            path_tracer.set_data(comp_data.data_array.as_array())

    # -- serde JSON (sdf_editor.rs:131-167) ----------------------------
    def to_json(self) -> dict:
        return {"header_unions": [u.to_json() for u in self.header_unions], "save_name": self.save_name}

    def dumps(self) -> str:
        return json.dumps(self.to_json(), indent=2)

    @classmethod
    def from_json(cls, d: dict) -> "SDFEditor":
        ed = cls([Union.from_json(u) for u in d["header_unions"]])
        ed.save_name = d.get("save_name", "")
        return ed

    @classmethod
    def loads(cls, s: str) -> "SDFEditor":
        return cls.from_json(json.loads(s))

    def rows(self) -> List[dict]:
        return flatten(self.header_unions)[0]

    def shape_nodes(self) -> List[Shape]:
        """The tree's shapes in the order of the compiled program's
        PT_OP_SHAPE ops: element k is the node behind shape ordinal k (what
        ``PathTracer.pick`` / ``trace_rays`` / ``sample_field`` and a mesh's
        ``shapes`` report).  The compiler emits a union's child unions, then
        its shapes -- ``flatten``'s order, which ``compile`` pairs with the
        shape ops one for one."""
        return [o for o in flatten(self.header_unions)[1] if isinstance(o, Shape)]
