"""Writes tests/golden/program_digests.json and tests/golden/editor_save.json:
what the editor mirror compiles, saves and flattens, recorded so that
tests/test_editor_pins.py holds a later restatement of sdf_editor.py to it.

* program_digests.json -- for every scenes.SCENES entry and every
  fuzz_scene(seed) of scenes.FUZZ_SEEDS: the counts of the compiled Program
  and the sha256 of ops + aabbs + data + str(n_check) (test_editor_pins.program_record);
  for c2 and nested also the sha256 of json.dumps of op_dicts() / aabb_dicts().
  The Floats' random hashes reach none of it.
* editor_save.json -- "editor": the parsed dumps() of a small tree with fixed
  hashes (editor_tree below), "dumps_sha256": the sha256 of that text (so
  json.dumps(editor, indent=2) is dumps() byte for byte), "rows_sha256": the
  sha256 of json.dumps(rows()), "plane": the to_json() of one Plane shape.

Needs the built library.  Run: python tests/golden/make_editor_pins.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from compute_path_tracer_amd.sdf_editor import CompData, SDFEditor, Shape, Shapes, Union, UnionType  # noqa: E402
from test_editor_pins import program_record, scene_makers, sha  # noqa: E402  (the records as the test forms them)


def fixed_hash(k: int) -> int:
    return int.from_bytes(hashlib.sha256(b"editor_save:%d" % k).digest()[:16], "little")


def shape_of(kind: str, name: str, pos, size, **material) -> Shape:
    s = Shape(kind)
    s.name = name
    s.transform.position.set(pos)
    for p, v in zip(s.current_shape.params, size):
        p.set(v)
    for field, v in material.items():
        getattr(s.material, field).set(v)
    return s


def editor_tree() -> SDFEditor:
    """One header union of a sphere, a cube, a torus and an octahedron, with a
    child Subtraction union of two shapes; every Float's hash fixed, the cube's
    size y sharing the sphere's size hash."""
    top = Union()
    top.name = "top"
    top.transform.position.set((0.1, -0.2, 0.3))
    top.transform.rotation.set((0.0, 0.4, 0.0))
    top.transform.scale.set(0.9)
    top.children_shapes += [
        shape_of(Shapes.SPHERE, "sphere", (-1.0, 0.0, 0.5), (0.8,), color=(0.9, 0.2, 0.2), brightness=1.5),
        shape_of(Shapes.CUBE, "cube", (1.0, 0.1, 0.5), (0.5, 0.6, 0.7), specular_chance=0.5, roughness=0.25),
        shape_of(Shapes.TORUS, "torus", (0.0, 1.0, 0.0), (0.9, 0.2), color=(0.2, 0.3, 0.9)),
        shape_of(Shapes.OCTAHEDRON, "octahedron", (0.0, -1.0, 0.2), (0.7,), light_col=(1.0, 0.8, 0.6), brightness=2.0),
    ]
    top.children_shapes[1].transform.rotation.set((0.3, 0.0, -0.2))
    top.children_shapes[2].transform.aabb = False
    cut = Union(UnionType.SUBTRACTION)
    cut.name = "cut"
    cut.transform.position.set((0.0, 0.0, 1.5))
    cut.transform.aabb_exaggeration.set(2.0)
    cut.children_shapes += [
        shape_of(Shapes.CUBE, "block", (0.0, 0.0, 0.0), (0.6, 0.6, 0.6), color=(0.5, 0.5, 0.5)),
        shape_of(Shapes.SPHERE, "hole", (0.2, 0.2, -0.2), (0.5,), refract_chance=0.3, ior=1.4),
    ]
    cut.children_shapes[1].transform.scale.set(1.1)
    top.children_unions.append(cut)
    ed = SDFEditor([top])
    ed.save_name = "editor_save"
    k = 0
    for u in (top, cut):
        for f in (*u.transform.floats(), *(f for s in u.children_shapes for f in s.floats())):
            f.hash = fixed_hash(k)
            k += 1
    sphere, cube = top.children_shapes[:2]
    cube.current_shape.params[1].hash = sphere.current_shape.params[0].hash
    return ed


def plane_shape() -> Shape:
    s = shape_of(Shapes.PLANE, "plane", (0.0, -2.0, 0.0), (), color=(0.4, 0.6, 0.4))
    for k, f in enumerate(s.floats()):
        f.hash = fixed_hash(1000 + k)
    return s


def main() -> None:
    digests = {name: program_record(name, make().compile(CompData())) for name, make in scene_makers().items()}
    with open(os.path.join(HERE, "program_digests.json"), "w") as f:
        json.dump(digests, f, indent=1)
        f.write("\n")
    ed = editor_tree()
    text = ed.dumps()
    save = {"editor": json.loads(text), "dumps_sha256": sha(text),
            "rows_sha256": sha(json.dumps(SDFEditor.loads(text).rows())), "plane": plane_shape().to_json()}
    with open(os.path.join(HERE, "editor_save.json"), "w") as f:
        json.dump(save, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
