"""Distance-bound culling of the scene kernels, host side.

The bound data (PtNode.pad[0], pt_derive.cpp pt_cull_bounds) is read back
from the values-baked hipRTC source (exact hex literals) and recomputed here
from the same baked node values; the generated map() must carry the parent
rule exactly for the unions the rule allows.  No GPU: hipRTC cross-compiles.
The numerics -- every map() variant and bounds() against the oracle, point by
point -- are checked on the GPU by test_gpu_map.py; the
exactness of the culled images by test_gpu_parity.py (scene "cull" and every
scene with eligible unions)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from compute_path_tracer_amd import _native as N, scenes
from compute_path_tracer_amd.sdf_editor import CompData


def _value(tok: str) -> float:
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


def _baked(scene: str, tmp_path):
    """The values-baked scene kernel source (pt_scene_kernel_source: generated,
    not compiled) and its node literals."""
    src = N.scene_kernel_source(scenes.SCENES[scene]().compile(CompData()), baked=1)
    nodes = []
    # the node literals of the first map (JitMap); JitMapB repeats them
    for m in re.finditer(r"constexpr PtNode B(\d+)\{(.*?)\};\n", src[:src.index("struct JitMapB")]):
        toks = [t for t in m.group(2).replace("{", ",").replace("}", ",").split(",") if t.strip()]
        v = [_value(t) for t in toks]
        nodes.append(dict(op=int(v[0]), shape=int(v[1]), combine=int(v[2]), inv=v[6], m=v[7:10], rot=v[10:16],
                          size=v[16:19], pad=v[19]))
        assert int(m.group(1)) == len(nodes) - 1
    return src, nodes


@pytest.mark.parametrize("scene", sorted(scenes.SCENES))
def test_kernel_source_two_call_sizes(scene):
    """pt_scene_kernel_source's two-call pattern: the first call reports the
    bytes including the terminating NUL, a buffer one byte short is
    PT_ERR_SIZE, and the full one holds exactly the reported text."""
    prog = scenes.SCENES[scene]().compile(CompData())
    args = (prog.ops, prog.n_ops, prog.aabbs, prog.n_aabb, prog.data.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
            len(prog.data), 1)
    n = ctypes.c_size_t()
    assert N.lib().pt_scene_kernel_source(*args, None, 0, ctypes.byref(n)) == N.PT_OK
    buf = ctypes.create_string_buffer(n.value)
    assert N.lib().pt_scene_kernel_source(*args, buf, n.value - 1, ctypes.byref(n)) == N.PT_ERR_SIZE
    assert N.lib().pt_scene_kernel_source(*args, buf, n.value, ctypes.byref(n)) == N.PT_OK
    src = buf.value.decode()
    assert len(src) + 1 == n.value


def _expected_shape_pad(n) -> float:
    """pt_cull_bounds for one shape (R' = R + 2^-12 (|R| + |m|_1), or NaN)."""
    big = 2.0 ** 40
    fin = lambda v: math.isfinite(v) and abs(v) <= big  # noqa: E731
    ok = math.isfinite(n["inv"]) and 2.0 ** -20 <= n["inv"] <= 2.0 ** 20 and all(map(fin, n["m"] + n["rot"]))
    s = n["size"]
    if n["shape"] == N.PT_NODE_SPHERE:
        ok, R = ok and fin(s[0]), s[0]
    elif n["shape"] == N.PT_NODE_CUBE:
        ok = ok and all(fin(x) and x >= 0.0 for x in s)
        R = math.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
    elif n["shape"] == N.PT_NODE_TORUS:
        ok, R = ok and fin(s[0]) and fin(s[1]), abs(s[0]) + s[1]
    elif n["shape"] == N.PT_NODE_OCTAHEDRON:
        ok, R = ok and fin(s[0]) and s[0] >= 0.0, s[0]
    else:
        ok, R = False, 0.0
    if not ok:
        return math.nan
    return float(np.float32(R + 2.0 ** -12 * (abs(R) + sum(abs(x) for x in n["m"]))))


def _same(a: float, b: float) -> bool:
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("scene", ["cull", "c3", "c2", "nested"])
def test_bounds_match_restatement(scene, tmp_path):
    src, nodes = _baked(scene, tmp_path)
    assert nodes
    # parent accumulator still MAXHIT when the union begins (no cull code then)
    fresh_parent, fresh = {}, [True]
    for i, n in enumerate(nodes):
        if n["op"] == N.PT_OP_UNION_BEGIN:
            fresh_parent[i] = fresh[-1]
            fresh.append(True)
        elif n["op"] == N.PT_OP_SHAPE:
            fresh[-1] = False
        else:
            fresh.pop()
            fresh[-1] = False
    assert any(fresh_parent.values())  # the first header union
    src, src_b = src[:src.index("struct JitMapB")], src[src.index("struct JitMapB"):]
    # JitMapB's bound rule: top-level unions whose later
    # top-level combines are all unions
    top, depth = [], 0
    for i, n in enumerate(nodes):
        if n["op"] == N.PT_OP_UNION_BEGIN:
            if depth == 0:
                start = i
            depth += 1
        elif n["op"] == N.PT_OP_UNION_END:
            depth -= 1
            if depth == 0:
                top.append((start, n["combine"]))
    use_bnd, later = {}, True
    for start, comb in reversed(top):
        use_bnd[start] = later
        later = later and comb == N.PT_COMBINE_UNION
    for i, n in enumerate(nodes):
        if n["op"] == N.PT_OP_SHAPE:
            assert _same(n["pad"], _expected_shape_pad(n)), (i, n)
        elif n["op"] == N.PT_OP_UNION_BEGIN:
            j, ok = i + 1, True
            while nodes[j]["op"] != N.PT_OP_UNION_END:
                c = nodes[j]
                if c["op"] != N.PT_OP_SHAPE or c["combine"] not in (N.PT_COMBINE_ASSIGN, N.PT_COMBINE_UNION) \
                        or math.isnan(c["pad"]):
                    ok = False
                j += 1
            e = nodes[j]
            ok = ok and e["combine"] == N.PT_COMBINE_UNION and math.isfinite(e["inv"]) and e["inv"] > 0.0
            assert _same(n["pad"], e["inv"] if ok else math.nan), (i, n)
            # the rule is emitted exactly for the structurally eligible unions
            # that have a running parent distance to test against
            static = all(nodes[k]["op"] == N.PT_OP_SHAPE and nodes[k]["combine"] != N.PT_COMBINE_SUBTRACTION
                         for k in range(i + 1, j)) and e["combine"] == N.PT_COMBINE_UNION and not fresh_parent[i]
            # (the trace map's target carries the NaN-folded point bound:
            # `pb ? h.d * B.pad[0] : NaN`, PT_JIT_PBNAN)
            assert (f"* B{i}.pad[0]" in src) == static, i
            eligible = static or (fresh_parent[i] and use_bnd.get(i, False) and all(
                nodes[k]["op"] == N.PT_OP_SHAPE and nodes[k]["combine"] != N.PT_COMBINE_SUBTRACTION
                for k in range(i + 1, j)) and e["combine"] == N.PT_COMBINE_UNION)
            assert (f"* B{i}.pad[0];" in src_b) == eligible, i
            assert (f"cull_target(h0.d, bnd) * B{i}.pad[0];" in src_b) == (eligible and use_bnd.get(i, False)), i
        else:
            assert math.isnan(n["pad"])


def test_cull_scene_switches_the_rule_off_where_values_demand(tmp_path):
    _, nodes = _baked("cull", tmp_path)
    begins = [i for i, n in enumerate(nodes) if n["op"] == N.PT_OP_UNION_BEGIN]
    # header unions: room, objects-a, objects-b (subtraction), objects-c, cluster-0..5
    pads = [nodes[i]["pad"] for i in begins]
    assert len(pads) == 10
    assert math.isnan(pads[2])  # subtraction union
    assert math.isnan(pads[7])  # cluster-3: a cube with a negative size
    assert math.isnan(pads[8])  # cluster-4: a shape with 1/s beyond 2^20
    assert all(math.isfinite(p) for k, p in enumerate(pads) if k not in (2, 7, 8))
    neg = [n for n in nodes if n["op"] == N.PT_OP_SHAPE and n["shape"] == N.PT_NODE_SPHERE and n["size"][0] < 0]
    assert neg and all(math.isfinite(n["pad"]) for n in neg)  # R = r < 0 still bounds a sphere


def test_dropped_assign_shape_stands_in_as_inf(tmp_path):
    """A union's first shape is combined by assignment (containers.rs:244-252),
    which overwrites MAXHIT.  When the cull drops it, the scene kernel must not
    leave MAXHIT * s (10 world units at scale 1e-3, which would beat a larger
    parent distance): it assigns +inf, a value above the cull target as the
    dropped shape's own was.  The speck unions of scene "tiny" are cull-eligible."""
    src, nodes = _baked("tiny", tmp_path)
    begins = [i for i, n in enumerate(nodes) if n["op"] == N.PT_OP_UNION_BEGIN]
    assert len(begins) == 3 and all(math.isfinite(nodes[i]["pad"]) for i in begins[1:])
    for b in begins[1:]:
        first = b + 1
        assert nodes[first]["combine"] == N.PT_COMBINE_ASSIGN
        mat_tag = f"h1 = Hit{{__builtin_inff(), "
        body = src[src.index(f"// shape {first}\n"):]
        body = body[:body.index("    }\n")]
        assert "if (cut) " + mat_tag in body, body
    # JitMapB1's whole-union skip (live mask) assigns +inf too
    b1 = src[src.index("struct JitMapB1"):]
    assert b1.count("} else {  // live") >= 1
    live = b1[b1.index("} else {  // live"):]
    assert live[:live.index("if constexpr")].count("= Hit{__builtin_inff(), ") == 1


def test_far_box_takes_the_ieee_bounds_path(tmp_path):
    """A box coordinate beyond the reciprocal guard (scene "farbox", 1e20)
    makes the values-baked shade kernel's bounds() select its IEEE-division
    branch for every ray; the GPU parity test runs it."""
    src, _ = _baked("farbox", tmp_path)
    assert "const bool fast = false && " in src
    src_c2, _ = _baked("c2", tmp_path)
    assert "const bool fast = true && " in src_c2


@pytest.mark.parametrize("scene,wide", [("c3", 0), ("wide", 1)])
def test_check_width_is_a_compile_time_constant(scene, wide, tmp_path):
    """MapWide: a scene whose check[] indices stay below 64 gets kernels
    without the high mask words; a wider one keeps them (pt_jit.cpp)."""
    src, _ = _baked(scene, tmp_path)
    for m in ("JitMap", "JitTaps"):
        assert f"template <> struct MapWide<{m}> {{\n  static constexpr int v = {wide};" in src


def test_material_table_size_and_scale_reciprocals(tmp_path):
    """The shade pass's LDS material table covers every material a shape can
    name, and each baked scale division uses the correctly rounded reciprocal
    of its divisor (pt_div_k)."""
    src, nodes = _baked("c3", tmp_path)
    prog = scenes.SCENES["c3"]().compile(CompData())
    n_mat = int(re.search(r"struct MapMats<JitTaps> \{\n  static constexpr int n = (\d+);", src).group(1))
    shapes = [m for m in re.finditer(r"constexpr PtNode B\d+\{1, \d+, \d+, -?\d+, (\d+),", src[:src.index("struct JitMapB")])]
    assert n_mat == 1 + max(int(m.group(1)) for m in shapes)
    calls = re.findall(r"pt_div_k\(d, B(\d+)\.inv, ([^)]+)\)", src)
    assert calls, "C3's scaled unions divide by their scale constants"
    for i, y in calls:
        inv = np.float32(nodes[int(i)]["inv"])
        assert np.float32(_value(y)) == np.float32(1.0) / inv
    assert prog.n_ops > 0


def test_radius_test_and_bounds_forms(tmp_path):
    """The shipped codegen choices (DESIGN.md 5 history, 3.19): the radius
    cull test joins its point bound with `&` (no exec-mask region around the
    test), and the shade kernels' straight-line bounds() decides its slab
    tests by the ulp margin, one select per box bit."""
    src, _ = _baked("c3", tmp_path)
    trace, taps = src[:src.index("struct JitMapB")], src[src.index("struct JitMapB"):]
    # the trace map: the point bound folded into the union's target as NaN
    # (PT_JIT_PBNAN), the target's margin term hoisted per union
    assert re.search(r"const float tg\d+ = pb\d+ \? h\d+\.d \* B\d+\.pad\[0\] : __builtin_nanf\(\"\"\);", trace)
    assert re.search(r"const float cT\d+ = __builtin_fmaf\(fabsf\(tg\d+\), 0x1p-12f, tg\d+\);", trace)
    assert re.findall(r"const bool cut = cl \* 0x1\.ff8p-1f > cK \* cK;", trace)
    assert not re.findall(r"const bool cut = pb\d+", trace)
    cuts = re.findall(r"const bool cut = pb\d+ (&&?) \(cl \* 0x1\.ff8p-1f > cK \* cK\);", taps)
    assert cuts and set(cuts) == {"&"}, set(cuts)
    assert "uint32_t gapu = 0xffffffffu;" in src
    assert "__ballot(!(gapu > PT_ULP_MARGIN))" in src
    assert re.search(r"w0 \|= ray_box_ulp\(A0, ro\.x, ro\.y, ro\.z, yx, yy, yz, gapu\) \? 0x[0-9a-f]+u : 0u;", src)


def test_run_cut_carries_the_underflow_guard(tmp_path):
    """The trace map's run cut (a cube joining its union by min is skipped
    when max(q) exceeds the running distance) relies on sdCube >= max(q),
    which holds in f32 only for max(q) > 2^-60: every run
    cut the generator emits must carry that guard, like cut_q does."""
    src, _ = _baked("c3", tmp_path)
    runs = re.findall(r"const bool cut_r = \(qm > h\d+\.d\)( & \(qm > 0x1p-60f\))?;", src)
    assert runs, "C3's room cubes take the run cut"
    assert all(g for g in runs), runs
    assert not re.search(r"if \(!?\(?qm > h\d+\.d\)", src)
    assert all("qm > 0x1p-60f" in m for m in re.findall(r"const bool cut_q = [^;]*;", src))


def _compile_log(scene: str) -> str:
    prog = scenes.SCENES[scene]().compile(CompData())
    old = os.environ.get("PT_JIT_BAKE")
    os.environ["PT_JIT_BAKE"] = "1"
    try:
        log = ctypes.create_string_buffer(1 << 16)
        rc = N.lib().pt_jit_compile(prog.ops, prog.n_ops, prog.aabbs, prog.n_aabb,
                                    prog.data.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(prog.data), log,
                                    len(log), None)
    finally:
        if old is None:
            os.environ.pop("PT_JIT_BAKE", None)
        else:
            os.environ["PT_JIT_BAKE"] = old
    assert rc == N.PT_OK, log.value.decode()
    return log.value.decode(errors="replace")


@pytest.mark.parametrize("scene,fallback", [("c3", False), ("wide", True)])
def test_spilling_build_falls_back_to_seven_waves(scene, fallback, tmp_path):
    """The scene kernels are built for 8 waves per SIMD (64 VGPRs); a build
    whose trace kernels spill, or whose shade kernel spills more than 16 bytes
    per lane, is rebuilt at 7 (pt_jit_build.cpp pt_jit_compile_source).  C3 keeps
    the 8-wave build; the 128-entry `wide` scene spills and falls back."""
    src, _ = _baked(scene, tmp_path)
    assert "#define PT_TW_N 8" in src and "#define PT_SW_N 8" in src
    assert "amdgpu_waves_per_eu(PT_TW_N)" in src
    # (in a fresh process: one that imported torch first compiles with torch's
    # bundled hipRTC / comgr, whose allocation spills C3 at 8 waves -- DESIGN.md 5)
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    prog = (f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; "
            f"import test_cull as T; print(T._compile_log({scene!r}).splitlines()[0])")
    out = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("(rebuilt at 7 waves per SIMD") == fallback, out.stdout[:500]



_PROBE = r"""
import ctypes, os, sys
if sys.argv[2] == "torch":
    import torch  # noqa: F401 -- torch's bundled hipRTC / comgr are loaded first
sys.path.insert(0, sys.argv[1])
from compute_path_tracer_amd import _native as N, scenes
from compute_path_tracer_amd.sdf_editor import CompData
os.environ["PT_JIT_BAKE"] = sys.argv[4]
p = scenes.SCENES[sys.argv[3]]().compile(CompData())
log = ctypes.create_string_buffer(1 << 16)
size = ctypes.c_size_t()
rc = N.lib().pt_jit_compile(p.ops, p.n_ops, p.aabbs, p.n_aabb, p.data.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                            len(p.data), log, len(log), ctypes.byref(size))
print(rc, int(log.value.startswith(b"(rebuilt")), size.value)
"""


def _probe(scene: str, bake: str, first: str = "none", **env):
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = {k: v for k, v in os.environ.items() if not k.startswith("PT_JIT")}
    e.update(env)
    out = subprocess.run([sys.executable, "-c", _PROBE, root, first, scene, bake], capture_output=True, text=True,
                         timeout=900, env=e)
    assert out.returncode == 0, out.stderr[-2000:]
    rc, rebuilt, size = out.stdout.split()[-3:]
    assert rc == "0"
    return rebuilt == "1", int(size)


def test_jit_disk_cache_round_trip(tmp_path):
    """pt_jit_build.cpp's on-disk cache: PT_JIT_CACHE=2 writes one entry per
    generated source, a later process reads the same code object back, and a
    compile knob that changes the build changes the key (a miss)."""
    d = str(tmp_path)
    _, size = _probe("c1", "1", PT_JIT_CACHE="2", PT_JIT_CACHE_DIR=d)
    files = sorted(os.listdir(d))
    assert len(files) == 1 and files[0].endswith(".ptjit")
    path = os.path.join(d, files[0])
    with open(path, "rb") as f:
        assert f.read(8) == b"PTJIT2\0\0"
    assert _probe("c1", "1", PT_JIT_CACHE="1", PT_JIT_CACHE_DIR=d)[1] == size
    # a damaged entry is a miss (checksum), not a broken kernel: the scene compiles
    with open(path, "r+b") as f:
        f.seek(-100, 2)
        f.write(b"\xff" * 8)
    assert _probe("c1", "1", PT_JIT_CACHE="1", PT_JIT_CACHE_DIR=d)[1] == size
    _probe("c1", "1", PT_JIT_CACHE="2", PT_JIT_CACHE_DIR=d, PT_JIT_DEFS="PT_UNUSED_PROBE")
    assert len(os.listdir(d)) == 2


def test_shipped_scene_kernels_survive_a_torch_first_process():
    """A process that imported torch first holds torch's bundled, older
    hipRTC, whose register allocation makes C3's 8-wave build spill (the 7-wave
    rebuild runs 4-5 % slower).  build() ships the BASELINE
    scenes' kernels in lib/jitcache, compiled with this image's hipRTC, so that
    process still loads the 8-wave build; with the cache off it does not."""
    assert _probe("c3", "1", first="torch") == _probe("c3", "1", first="none")
    assert _probe("c3", "1", first="torch")[0] is False
    # (with the cache off, this image's torch compiles the 7-wave rebuild; not
    # asserted, as that is a property of torch's bundled compiler)


def test_wave_fallback_is_per_kernel():
    """pt_jit_build.cpp rebuilds at 7 waves only the kernels whose 8-wave build
    spilled (PT_TW_N: march-only trace, PT_TG_N: first pass, PT_TT_N: taps
    in the trace pass, PT_SW_N: shade beyond 16 bytes per lane); the log's
    first line names both lists, and they must agree.  C3's table build
    (values read from the node table) is the case that spills in part."""
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    prog = (f"import os, sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; os.environ['PT_JIT_CACHE'] = '0'; "
            f"import test_cull as T; T.os.environ['PT_JIT_BAKE'] = '0'; "
            f"import ctypes; from compute_path_tracer_amd import scenes, _native as N; "
            f"from compute_path_tracer_amd.sdf_editor import CompData; p = scenes.SCENES['c3']().compile(CompData()); "
            f"log = ctypes.create_string_buffer(1 << 16); "
            f"rc = N.lib().pt_jit_compile(p.ops, p.n_ops, p.aabbs, p.n_aabb, "
            f"p.data.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(p.data), log, len(log), None); "
            f"print(rc); print(log.value.decode(errors='replace').splitlines()[0])")
    out = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rc, first = out.stdout.splitlines()[-2:]
    assert rc == "0"
    if not first.startswith("(rebuilt at 7 waves per SIMD"):
        return  # (this compiler fits the whole table build in 64 VGPRs)
    m = re.match(r"\(rebuilt at 7 waves per SIMD:((?: PT_[A-Z]{2}_N=7)+); the 8-wave build spilled, bytes/lane:(.*)\)",
                 first)
    assert m, first
    lowered = set(m.group(1).split())
    spilled = dict(kv.split("=") for kv in m.group(2).split())
    want = set()
    for kernel, macro in (("pt_bin_trace_m_jit", "PT_TW_N"), ("pt_bin_trace_g_jit", "PT_TG_N"),
                          ("pt_bin_trace_jit", "PT_TT_N")):
        if int(spilled.get(kernel, 0)) > 0:
            want.add(macro + "=7")
    if int(spilled.get("pt_bin_shade_t_jit", 0)) > 16:
        want.add("PT_SW_N=7")
    assert lowered == want, (lowered, spilled)


@pytest.mark.parametrize("scene", ["c3", "wide"])
def test_primary_box_skip_guards(scene, tmp_path):
    """bounds()' fast path takes the first pass's box-skip hint (DESIGN.md
    3.20) as one guard per box below 64 -- primary_box_skip covers at most 64
    boxes, and a shift by 64 or more would be undefined (a 120-box scene's
    kernels faulted with such guards) -- and none above."""
    src, _ = _baked(scene, tmp_path)
    prog = scenes.SCENES[scene]().compile(CompData())
    shifts = [int(k) for k in re.findall(r"if \(!\(\(skip >> (\d+)\) & 1ull\)\)", src)]
    assert shifts == list(range(min(64, prog.n_aabb)))
    assert "mask_skip<ST>(L, ro, rd, 0ull, st)" in src  # the shade pass passes no hint
