#!/usr/bin/env python3
"""Digest of the generated scene-kernel source of every shipped scene: one
line `scene baked bytes sha256` per entry of scenes.SCENES and baked in (0, 1)
(the UTF-8 bytes without the terminating NUL).  The source is the scene
kernels' whole behaviour and, with the embedded headers, their cache key, so
equal digests before and after a change to the generator mean the same code
objects.  PT_LIB selects the library; PT_JIT_* knobs are dropped.  CPU only.
    python scripts/jit_source_digest.py [--dump DIR]   # DIR/<scene>.<baked>.hip for diff
"""
import hashlib
import os
import sys

for k in [k for k in os.environ if k.startswith("PT_JIT_")]:
    del os.environ[k]
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from compute_path_tracer_amd import _native as N, scenes  # noqa: E402
from compute_path_tracer_amd.sdf_editor import CompData  # noqa: E402

dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None
if dump:
    os.makedirs(dump, exist_ok=True)
for name, make in scenes.SCENES.items():
    prog = make().compile(CompData())
    for baked in (0, 1):
        raw = N.scene_kernel_source(prog, baked=baked).encode()
        print(f"{name:<9} {baked} {len(raw):6d} {hashlib.sha256(raw).hexdigest()}")
        if dump:
            with open(os.path.join(dump, f"{name}.{baked}.hip"), "wb") as f:
                f.write(raw)
