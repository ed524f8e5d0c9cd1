"""The scene-kernel generator (pt_jit.cpp) as text: generated, not compiled.
No GPU.  What the generated map() must contain is test_cull.py's subject; here:
the experiment hook, determinism, and the kernel entry points."""
import os
import re

import pytest

from compute_path_tracer_amd import _native as N, scenes
from compute_path_tracer_amd.sdf_editor import CompData


def _source(scene: str, baked: int) -> str:
    return N.scene_kernel_source(scenes.SCENES[scene]().compile(CompData()), baked=baked)


@pytest.mark.parametrize("baked", [0, 1])
def test_experiment_defines_follow_the_first_line(baked):
    """PT_JIT_DEFS="A,,B=1": empty tokens are skipped, `B=1` becomes
    `#define B 1`, and the defines stand right after the first comment line
    of an otherwise unchanged source."""
    old = os.environ.pop("PT_JIT_DEFS", None)
    try:
        plain = _source("c1", baked)
        os.environ["PT_JIT_DEFS"] = "A,,B=1"
        with_defs = _source("c1", baked)
    finally:
        if old is None:
            os.environ.pop("PT_JIT_DEFS", None)
        else:
            os.environ["PT_JIT_DEFS"] = old
    first, rest = plain.split("\n", 1)
    assert first.startswith("//")
    assert with_defs == first + "\n#define A\n#define B 1\n" + rest


@pytest.mark.parametrize("baked", [0, 1])
def test_generation_is_deterministic(baked):
    assert _source("c3", baked) == _source("c3", baked)


def test_every_kernel_is_defined_once():
    """The 14 scene kernels (pt_host.h PtJitFn): each an `extern "C"
    __global__` definition of its own in the generated source."""
    src = _source("wide", 1)
    names = re.findall(r'^extern "C" __global__ [^\n{]*?\bvoid (\w+)\(', src, re.M)
    assert len(names) == 14 and len(set(names)) == 14, names
    for name in names:
        assert len(re.findall(r"\b%s\b" % name, src)) == 1, name
