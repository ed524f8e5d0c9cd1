"""MI355X-native (gfx950) SDF sphere-trace + Monte-Carlo path-trace hot path.

Drop-in for the GLSL compute path of zachdedoo13/compute_path_tracer
(assets/shaders/path_tracer/test_compute.glsl dispatched by
src/path_tracer/path_tracer.rs).  The kernels live in ``csrc/`` and are reached
through the C ABI of ``include/pt_abi.h`` (``lib/libpt.so``); this package is the
host-side mirror of the reference's ``PathTracer`` and ``SDFEditor``.
"""
from .sdf_editor import CompData, Float, Material, SDFEditor, Shape, Shapes, Transform, Union, UnionType, V3  # noqa: F401
from ._native import Camera  # noqa: F401  (pt_camera: PathTracer.set_camera / look_at)
from ._native import Sky  # noqa: F401  (pt_sky: PathTracer.set_sky)
from .view import look_at_camera, preview_light, sky_light  # noqa: F401
from .mesh import Mesh, mesh_grid  # noqa: F401  (PathTracer.extract_mesh)

__all__ = ["Camera", "look_at_camera", "Sky", "sky_light", "preview_light", "Mesh", "mesh_grid","CompData", "Float", "Material", "SDFEditor", "Shape", "Shapes", "Transform", "Union", "UnionType", "V3"]
