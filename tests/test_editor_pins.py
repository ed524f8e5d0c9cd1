"""What the editor mirror compiles, saves and flattens, held to records made
before sdf_editor.py was restated (tests/golden/make_editor_pins.py):
every shipped scene's and every fuzz seed's compiled Program, the serde JSON
text of a small tree byte for byte, and that tree's flattened rows.  Host
only: pt_compile_scene_keyed needs no GPU."""
import ctypes
import hashlib
import json
import os

import pytest

from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.sdf_editor import CompData, SDFEditor, Shape

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DICT_FORM_SCENES = ("c2", "nested")


def sha(b) -> str:
    return hashlib.sha256(b if isinstance(b, bytes) else b.encode()).hexdigest()


def scene_makers() -> dict:
    """Every scenes.SCENES entry, and fuzz_scene(seed) for every scenes.FUZZ_SEEDS seed."""
    makers = dict(scenes.SCENES)
    makers.update({f"fuzz_scene({seed})": (lambda seed=seed: scenes.fuzz_scene(seed)) for seed in scenes.FUZZ_SEEDS})
    return makers


def program_record(name: str, prog) -> dict:
    """The counts of a Program and the sha256 of its ops, aabbs and data as
    raw bytes followed by str(n_check); for DICT_FORM_SCENES also the sha256
    of json.dumps of its dict forms."""
    ops = ctypes.string_at(prog.ops, prog.n_ops * ctypes.sizeof(prog.ops._type_))
    aabbs = ctypes.string_at(prog.aabbs, prog.n_aabb * ctypes.sizeof(prog.aabbs._type_))
    rec = {"n_ops": prog.n_ops, "n_aabb": prog.n_aabb, "n_data": len(prog.data), "n_check": prog.n_check,
           "digest": sha(ops + aabbs + prog.data.tobytes() + str(prog.n_check).encode())}
    if name in DICT_FORM_SCENES:
        rec["op_dicts"] = sha(json.dumps(prog.op_dicts()))
        rec["aabb_dicts"] = sha(json.dumps(prog.aabb_dicts()))
    return rec


def golden(name: str) -> dict:
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_every_scene_is_recorded():
    want = golden("program_digests.json")
    assert set(want) == set(scene_makers()) and len(want) == len(scenes.SCENES) + len(scenes.FUZZ_SEEDS) == 67
    assert all(("op_dicts" in rec) == (name in DICT_FORM_SCENES) for name, rec in want.items())


@pytest.mark.parametrize("name", list(scene_makers()))
def test_compiled_program_is_the_recorded_one(name):
    assert program_record(name, scene_makers()[name]().compile(CompData())) == golden("program_digests.json")[name]


def test_save_text_round_trips_byte_for_byte():
    """Key order and indentation of every to_json: the text is the recorded
    dumps(), and loading and saving it again changes nothing."""
    save = golden("editor_save.json")
    text = json.dumps(save["editor"], indent=2)
    assert sha(text) == save["dumps_sha256"]
    assert SDFEditor.loads(text).dumps() == text


def test_save_holds_what_it_is_meant_to():
    top, = golden("editor_save.json")["editor"]["header_unions"]
    assert [next(iter(s["current_shape"])) for s in top["children_shapes"]] == ["Sphere", "Cube", "Torus", "Octahedron"]
    cut, = top["children_unions"]
    assert cut["union_type"] == "Subtraction" and len(cut["children_shapes"]) == 2
    sphere, cube = top["children_shapes"][:2]
    assert sphere["current_shape"]["Sphere"]["hash"] == cube["current_shape"]["Cube"]["y"]["hash"]
    assert sphere["current_shape"]["Sphere"]["val"] != cube["current_shape"]["Cube"]["y"]["val"]


def test_plane_shape_round_trips():
    plane = golden("editor_save.json")["plane"]
    assert plane["current_shape"] == "Plane"
    assert Shape.from_json(plane).to_json() == plane
    assert json.dumps(Shape.from_json(plane).to_json()) == json.dumps(plane)  # (key order too)


def test_rows_of_the_loaded_save():
    """With loaded hashes the rows are deterministic, keys included."""
    save = golden("editor_save.json")
    rows = SDFEditor.loads(json.dumps(save["editor"])).rows()
    assert sha(json.dumps(rows)) == save["rows_sha256"]
    assert [list(r) for r in rows] == [["kind", "parent", "union_type", "aabb", "scale", "position", "rotation",
                                         "aabb_exaggeration", "size", "material", "keys"]] * 8
