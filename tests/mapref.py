"""Inputs and expected values of the point probes: where the
scene kernels' map() variants and bounds() are asked, and what the CPU oracle
answers there.  Shared by test_map_ref.py (no GPU) and test_gpu_map.py.

The reference is the C oracle, directly: pto_map(p, check) per point,
pto_bounds(ro, rd) per ray, the tap points as meshref.normal forms them.  The
families below are functions of (editor rows, seed); world positions of
shape-local points come from the rows' transform chain in float64 -- they are
only inputs, so that precision suffices.  Masks are uint64 [n][2]: check[]
bits 0..63 and 64..127."""
import ctypes
import functools
import re

import numpy as np

import fuzzref
import meshref
from compute_path_tracer_amd import _native as N, scenes
from compute_path_tracer_amd.sdf_editor import CompData
from oracle import oracle as O

F = np.float32
U64 = np.uint64
ALL = 0xFFFFFFFFFFFFFFFF
MASK_FAMILIES = ("ones", "zeros", "logged", "random", "single")
POINT_FAMILIES = ("specials", "box", "path", "around", "cube")
BOUND_FAMILIES = ("inf", "nan", "pipeline", "tightest")
LOG_W, LOG_H, LOG_SPP, LOG_BOUNCES = 16, 12, 2, 4  # the render whose segments are logged

EDITORS = dict(scenes.SCENES)
EDITORS.update({"chain8": lambda: fuzzref.chain_scene(8), "boxed72": lambda: fuzzref.boxed_scene(72),
                "nan-sphere": meshref.nan_sphere_scene, "inf-sphere": meshref.inf_sphere_scene})
# the scenes the GPU tests probe, and what each brings (the smallest with the feature)
GPU_SCENES = ("c2", "nested", "cull", "tiny", "farbox", "fuzz-56", "fuzz-15793", "chain8", "boxed72", "nan-sphere",
              "inf-sphere", "c3")


class Scene:
    """An editor tree with its oracle, its compiled program and its logged segments."""

    def __init__(self, ed):
        self.ed = ed
        self.rows = ed.rows()
        self.prog = ed.compile(CompData())
        self.osc = O.OracleScene(self.rows)
        self.n_check = self.osc.n_check
        self._ck = {}

    def check_array(self, lo, hi):
        """check[] as the oracle takes it, for the mask (lo, hi); built once per mask."""
        key = (int(lo), int(hi))
        if key not in self._ck:
            bits = [(key[k >> 6] >> (k & 63)) & 1 for k in range(max(1, self.n_check))]
            self._ck[key] = (ctypes.c_uint8 * max(1, self.n_check))(*bits)
        return self._ck[key]

    def map(self, points, masks):
        """pto_map per point under its own mask: (d float32 [n], node int32 [n], the oracle's numbering)."""
        p = np.ascontiguousarray(points, F).reshape(-1, 3)
        m = np.ascontiguousarray(masks, U64).reshape(-1, 2)
        d, node = np.empty(len(p), F), np.empty(len(p), np.int32)
        L, h, out = self.osc._L, self.osc._h, ctypes.c_int32()
        fp, base = ctypes.POINTER(ctypes.c_float), p.ctypes.data
        for i in range(len(p)):
            d[i] = L.pto_map(h, ctypes.cast(base + 12 * i, fp), self.check_array(m[i, 0], m[i, 1]), ctypes.byref(out))
            node[i] = out.value
        return d, node

    def bounds(self, ro, rd):
        """pto_bounds per ray as a mask: bit k = check[k]."""
        o = np.ascontiguousarray(ro, F).reshape(-1, 3)
        r = np.ascontiguousarray(rd, F).reshape(-1, 3)
        out = np.zeros((len(o), 2), U64)
        L, h = self.osc._L, self.osc._h
        ck, dbg = (ctypes.c_uint8 * max(1, self.n_check))(), (ctypes.c_float * 3)()
        fp = ctypes.POINTER(ctypes.c_float)
        for i in range(len(o)):
            L.pto_bounds(h, ctypes.cast(o.ctypes.data + 12 * i, fp), ctypes.cast(r.ctypes.data + 12 * i, fp), ck, dbg)
            for k in range(self.n_check):
                if ck[k]:
                    out[i, k >> 6] |= U64(1 << (k & 63))
        return out

    @functools.cached_property
    def segments(self):
        """The logged segments of the LOG render: (ro, rd, mask, seg, steps, hit)."""
        return O.logged_segments(self.osc, LOG_W, LOG_H, LOG_SPP, LOG_BOUNCES)

    @functools.cached_property
    def shapes(self):
        """One dict per shape row: its kind and size, its chain of (scale, position, rotation matrix) from
        the header union down to itself, its world scale, the radius bound R of DESIGN.md 3.12 in local
        units, its check[] bit (-1: none), and whether its union is cull-eligible."""
        out = []
        for i, r in enumerate(self.rows):
            if r["kind"] == N.PT_NODE_UNION:
                continue
            chain, j = [], i
            while j >= 0:
                chain.append(j)
                j = self.rows[j]["parent"]
            chain.reverse()
            tf = [(float(self.rows[k]["scale"]), np.array(self.rows[k]["position"], np.float64),
                   _rotation(self.rows[k]["rotation"])) for k in chain]
            world = float(np.prod([t[0] for t in tf]))
            s = [float(v) for v in r["size"]]
            R = {N.PT_NODE_SPHERE: abs(s[0]), N.PT_NODE_CUBE: float(np.sqrt(s[0] ** 2 + s[1] ** 2 + s[2] ** 2)),
                 N.PT_NODE_TORUS: abs(s[0]) + abs(s[1]), N.PT_NODE_OCTAHEDRON: abs(s[0])}[r["kind"]]
            out.append(dict(row=i, kind=r["kind"], size=s, chain=tf, world=world, R=R, union=r["parent"],
                            check=self.osc.node_slots(i)[1], eligible=self._eligible(r["parent"]),
                            fast_cube=r["kind"] == N.PT_NODE_CUBE and sorted(abs(v) for v in s)[1] * world >= 1.0))
        return out

    def _eligible(self, u):
        """The parent rule of 3.12 may apply to union row u: it joins its parent by union, has no child
        unions, and its shapes combine by assign / union."""
        rows = self.rows
        parent = rows[u]["parent"]
        joins_by_union = parent < 0 or rows[parent]["union_type"] == N.PT_UNION_TYPE_UNION
        no_child_unions = not any(r["parent"] == u and r["kind"] == N.PT_NODE_UNION for r in rows)
        return joins_by_union and no_child_unions and rows[u]["union_type"] == N.PT_UNION_TYPE_UNION

    @functools.cached_property
    def boxes(self):
        """bounds()' boxes, one per entry of the program's own box list and in its order, from the entry's
        data slots in float32 steps (aabb.glsl from_pos_size): (bmin [b][3], bmax [b][3]).
        test_map_ref.py pins them to the oracle's bounds()."""
        data = self.prog.data
        lo, hi = [], []
        with np.errstate(all="ignore"):
            for a in self.prog.aabb_dicts():
                c = np.array([data[k] for k in a["union_position"]], F) + np.array([data[k] for k in a["shape_position"]], F)
                s = [data[k] for k in a["size"]]
                so = {N.PT_SO_SCALAR: [s[0]] * 3, N.PT_SO_VEC3: s, N.PT_SO_TORUS: [s[0] + s[1], s[1], s[0] + s[1]]}.get(
                    a["so_kind"], [F(1.0)] * 3)
                hs = (np.array(so, F) * (data[a["union_scale"]] * data[a["shape_scale"]])) * data[a["aabb_exaggeration"]]
                lo.append(c - hs)
                hi.append(c + hs)
        return np.array(lo, F).reshape(-1, 3), np.array(hi, F).reshape(-1, 3)

    @functools.cached_property
    def backs(self):
        """The check[] entry of each box of `boxes`."""
        return [a["back"] for a in self.prog.aabb_dicts()]

    @functools.cached_property
    def generated(self):
        """What the scene's own generated map() says about itself, read from the baked probe source (the
        text the GPU tests run): `cull_unions`, the op index of every union whose shapes JitMap tests
        against its parent's running distance (a `tg` target) with the rule on by its values (the union's
        pad[0] of pt_cull_bounds is finite); `cull_off`, those with a target but the rule off; `live`,
        (live bit, check[] entry or -1) of every shape JitMapB0 records in `live`."""
        src = N.probe_kernel_source(self.prog, baked=1)
        a, b, c = (src.index("struct %s {" % v) for v in ("JitMap", "JitMapB0", "JitMapB1"))
        jm, b0 = src[a:b], src[b:c]
        pad = {int(i): v for i, v in re.findall(r"constexpr PtNode B(\d+)\{.*\{([^,{}]+), 0, 0, 0, 0\}\};", jm)}
        targets = [int(i) for i in re.findall(r"const float tg\d+ = [^;]*\bB(\d+)\.pad\[0\]", jm)]
        on = [i for i in targets if "nan" not in pad[i] and "inf" not in pad[i]]
        live = []
        for block in re.split(r"(?=\{  // shape \d+\n)", b0)[1:]:
            bit = re.search(r"live \|= 1ull << (\d+);", block)
            if bit:
                guard = re.search(r"if \(\(\(ck\.(lo|hi) >> (\d+)\) & 1ull\)\) $", b0[:b0.index(block)].rsplit("\n", 1)[1])
                live.append((int(bit.group(1)), -1 if not guard else int(guard.group(2)) + 64 * (guard.group(1) == "hi")))
        return dict(cull_unions=on, cull_off=[i for i in targets if i not in on], live=live)

    def expected_live(self, masks):
        """JitMapB0's `live` where its bound excludes nothing (+inf, or NaN: rule off) and the point is in
        range: the bit of every recorded shape whose check[] bit the lane has (3.13: a live bit is set only
        inside the shape's check[] test)."""
        m = np.ascontiguousarray(masks, U64).reshape(-1, 2)
        out = np.zeros(len(m), U64)
        for bit, k in self.generated["live"]:
            has = np.ones(len(m), bool) if k < 0 else ((m[:, k >> 6] >> U64(k & 63)) & U64(1)).astype(bool)
            out |= np.where(has, U64(1 << bit), U64(0))
        return out

    @functools.cached_property
    def row_of_op(self):
        """The editor row of every op (-1 for a union's end): both lists walk the tree in the same order."""
        out, r = [], 0
        for o in self.prog.op_dicts():
            out.append(-1 if o["opcode"] == N.PT_OP_UNION_END else r)
            r += o["opcode"] != N.PT_OP_UNION_END
        return out

    @functools.cached_property
    def bound_k(self):
        """pt_bound_k (pt_derive.cpp) restated: the scene's largest transform chain in world units, NaN: no bound."""
        data = self.prog.data
        K, scale, reach = 0.0, [1.0], [0.0]
        with np.errstate(all="ignore"):
            for o in self.prog.op_dicts():
                if o["opcode"] == N.PT_OP_UNION_END:
                    if len(scale) > 1:
                        scale.pop(), reach.pop()
                    continue
                inv = F(1.0) / data[o["scale"]]
                m = [data[k] * inv for k in o["position"]]
                size = [data[k] for k in o["size"]] if o["opcode"] == N.PT_OP_SHAPE else [F(0.0)] * 3
                if not (np.isfinite(inv) and 0.5 <= inv <= 2.0):
                    return F(np.nan)
                if not all(np.isfinite(v) and abs(float(v)) <= 1048576.0 for v in m + size):
                    return F(np.nan)
                sc = scale[-1] / float(inv)
                r = reach[-1] + (abs(float(m[0])) + abs(float(m[1])) + abs(float(m[2]))) * sc
                if o["opcode"] == N.PT_OP_UNION_BEGIN:
                    scale.append(sc), reach.append(r)
                    continue
                s = [float(v) for v in size]
                R = {N.PT_NODE_SPHERE: abs(s[0]), N.PT_NODE_CUBE: float(np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])),
                     N.PT_NODE_TORUS: abs(s[0]) + abs(s[1]), N.PT_NODE_OCTAHEDRON: abs(s[0])}[o["shape"]]
                K = max(K, r + R * sc)
        return F(K * (1.0 + 2.0 ** -20))


@functools.lru_cache(maxsize=None)
def scene(name) -> Scene:
    return Scene(EDITORS[name]())


def _rotation(rot):
    """rot3D's matrix Mz My Mx (oracle/pt_oracle.c rot3d, column-major constructors) in float64."""
    (cx, sx), (cy, sy), (cz, sz) = ((np.cos(a), np.sin(a)) for a in np.asarray(rot, np.float64))
    mx = np.array([1, 0, 0, 0, cx, -sx, 0, sx, cx], np.float64).reshape(3, 3).T
    my = np.array([cy, 0, sy, 0, 1, 0, -sy, 0, cy], np.float64).reshape(3, 3).T
    mz = np.array([cz, -sz, 0, sz, cz, 0, 0, 0, 1], np.float64).reshape(3, 3).T
    return mz @ my @ mx


def to_world(shape, local):
    """World positions of shape-local points: each transform is q = M (p / s - pos / s), so p = s M^T q + pos."""
    p = np.asarray(local, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for s, pos, M in reversed(shape["chain"]):
            p = s * (p @ M) + pos  # (rows of p times M = M^T applied to each)
    return p


def to_local(shape, world):
    p = np.asarray(world, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for s, pos, M in shape["chain"]:
            p = ((p - pos) / s) @ M.T
    return p


def usable(points):
    """Points as float32 with finite magnitudes at most 1e30 (next to f32's largest value
    a rotation's sum overflows and the reference's full matrices then make NaNs the kernels do not)."""
    with np.errstate(all="ignore"):
        p = np.asarray(points, np.float64).reshape(-1, 3)
        p = p[(np.isfinite(p) & (np.abs(p) <= 1e30)).all(-1)]
        return p.astype(F)


# ---- point families -----------------------------------------------------------------
def specials():
    """The thirteen of test_gpu_mesh.sample_points."""
    nan, inf = float("nan"), float("inf")
    return np.array([(0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.5), (1e6, -2e6, 3e6), (1e20, 0.0, 0.0),
                     (-1e30, 2e30, 3e30), (nan, 0.0, 0.0), (0.3, nan, 0.1), (nan, nan, nan), (inf, 0.0, 0.0),
                     (0.5, -inf, 0.25), (inf, -inf, inf), (1e-30, 1e-38, -1e-45)], F)


def box_points(seed, n=160):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-3, 3, (n, 3)), rng.uniform(-12, 12, (n, 3))]).astype(F)


def march(sc, ro, rd, mask, mhd, steps=80):
    """A sphere trace under `mask` in CastRay's float32 steps, p = ro + rd t, t += map(p): the march points,
    map values and ray parameters after each step, and whether it ended with |d| < `mhd`.  Only a source of
    inputs: unlike the pipeline's after_map it reports |d| < mhd beyond the far plane as an end too (the
    pipeline calls that a miss); every hit taken from it is checked against the oracle's |F| < 1e-4."""
    ro, rd = np.asarray(ro, F), np.asarray(rd, F)
    t, pts, ds, ts = F(0.0), [], [], []
    with np.errstate(all="ignore"):
        for _ in range(steps):
            p = (ro + rd * t).astype(F)
            d = sc.map(p, mask)[0][0]
            t = F(t + d)
            pts.append(p), ds.append(d), ts.append(t)
            if abs(d) < mhd:
                return np.array(pts, F), np.array(ds, F), np.array(ts, F), True
            if not t <= F(100.0):  # (t > FP, or a NaN)
                break
    return np.array(pts, F).reshape(-1, 3), np.array(ds, F), np.array(ts, F), False


@functools.lru_cache(maxsize=None)
def path_points(name, n_segments=48):
    """The march points of the first logged segments, each with its segment's own mask."""
    sc = scene(name)
    ro, rd, mask = sc.segments[:3]
    pts, masks = [np.zeros((0, 3), F)], [np.zeros((0, 2), U64)]
    for i in range(min(n_segments, len(ro))):
        p = march(sc, ro[i], rd[i], mask[i], F(0.001))[0]
        pts.append(p), masks.append(np.repeat(mask[i][None], len(p), 0))
    p, m = np.concatenate(pts), np.concatenate(masks)
    ok = np.isfinite(p).all(-1)
    return p[ok], m[ok]


def around_points(sc, seed, per_shape=24):
    """Around each shape: local directions uniform on the sphere at radii on a geometric grid from R / 4
    to 64 R (across every parent-rule and bound-rule threshold), the local origin, and points on the
    shape's own surface (|F_S| below 1e-4: found by bisection along the direction).  Returns (points,
    shape index per point, local radius / R per point)."""
    rng = np.random.default_rng(seed)
    pts, which, ratio = [], [], []
    for k, s in enumerate(sc.shapes):
        R = s["R"]
        if not (np.isfinite(R) and R > 0 and np.isfinite(s["world"]) and s["world"] > 0):
            R = 1.0
        v = rng.normal(size=(per_shape, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        rad = R * 0.25 * (256.0 ** (np.arange(per_shape) / (per_shape - 1)))
        local = np.concatenate([v * rad[:, None], np.zeros((1, 3)), surface_points(s, v[:6])])
        pts.append(to_world(s, local))
        which += [k] * len(local)
        ratio += list(np.linalg.norm(local, axis=1) / R)
    if not pts:
        return np.zeros((0, 3), F), np.zeros(0, np.int64), np.zeros(0)
    p = np.concatenate(pts)
    ok = (np.isfinite(p) & (np.abs(p) <= 1e30)).all(-1)
    return p[ok].astype(F), np.array(which)[ok], np.array(ratio)[ok]


def local_sdf(shape, q):
    """The shape's exact SDF at local points, float64."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    s, kind = shape["size"], shape["kind"]
    if kind == N.PT_NODE_SPHERE:
        return np.linalg.norm(q, axis=1) - s[0]
    if kind == N.PT_NODE_CUBE:
        a = np.abs(q) - np.array(s)
        return np.linalg.norm(np.maximum(a, 0.0), axis=1) + np.minimum(a.max(1), 0.0)
    if kind == N.PT_NODE_TORUS:
        return np.hypot(np.hypot(q[:, 0], q[:, 2]) - s[0], q[:, 1]) - s[1]
    # octahedron: the face planes' distance (the sign, and the exact value near a face: all bisection needs)
    return (np.abs(q).sum(1) - s[0]) * 0.57735027


def surface_points(shape, dirs):
    """Local points on the shape's surface along `dirs` from the origin (bisection on the exact SDF;
    a direction without a sign change -- a torus's axis, a degenerate size -- gives its far end)."""
    R = shape["R"] if np.isfinite(shape["R"]) and shape["R"] > 0 else 1.0
    lo, hi = np.zeros(len(dirs)), np.full(len(dirs), 2.0 * R)
    if shape["kind"] == N.PT_NODE_TORUS:  # start on the ring's centre circle, go outwards
        base = np.array(dirs) * [1, 0, 1]
        base = base / np.maximum(np.linalg.norm(base, axis=1), 1e-30)[:, None] * shape["size"][0]
    else:
        base = np.zeros((len(dirs), 3))
    with np.errstate(all="ignore"):
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            inside = local_sdf(shape, base + np.array(dirs) * mid[:, None]) < 0.0
            lo, hi = np.where(inside, mid, lo), np.where(inside, hi, mid)
    return base + np.array(dirs) * hi[:, None]


def cube_points(sc, seed):
    """For every cube, local points above a face (exactly one positive q = |p| - b), above an edge (two),
    above a corner (three), inside, and on the qm = 0 surface.  Returns (points, cube's shape index,
    feature name per point)."""
    rng = np.random.default_rng(seed)
    pts, which, what = [], [], []
    for k, s in enumerate(sc.shapes):
        b = np.array(s["size"], np.float64)
        if s["kind"] != N.PT_NODE_CUBE or not (np.isfinite(b).all() and (b > 0).all()):
            continue
        for feature, npos in (("face", 1), ("edge", 2), ("corner", 3), ("inside", 0), ("surface", -1)):
            for _ in range(4):
                sign = rng.choice([-1.0, 1.0], 3)
                q = -b * rng.uniform(0.1, 0.9, 3)  # every axis inside
                if npos > 0:
                    axes = rng.permutation(3)[:npos]
                    q[axes] = b.min() * rng.uniform(0.05, 1.5, npos)
                elif npos < 0:
                    q[rng.integers(3)] = 0.0
                pts.append(sign * (q + b))
                which.append(k), what.append(feature)
    if not pts:
        return np.zeros((0, 3), F), np.zeros(0, np.int64), []
    world = np.concatenate([to_world(sc.shapes[k], p[None]) for k, p in zip(which, pts)])
    return world.astype(F), np.array(which), what


# ---- masks -----------------------------------------------------------------------------
def mask_family(sc, family, n, seed):
    """n masks of one family (bits beyond n_check are clear, as bounds() leaves them)."""
    rng = np.random.default_rng(seed)
    nc = sc.n_check
    valid = np.array([(1 << min(nc, 64)) - 1, (1 << max(nc - 64, 0)) - 1], dtype=U64)
    if family == "ones":
        return np.repeat(valid[None], n, 0)
    if family == "zeros":
        return np.zeros((n, 2), U64)
    if family == "logged":
        m = sc.segments[2]
        return m[rng.integers(len(m), size=n)] if len(m) else np.zeros((n, 2), U64)
    if family == "random":
        return rng.integers(0, 1 << 63, (n, 2), dtype=np.int64).astype(U64) * U64(2) + \
            rng.integers(0, 2, (n, 2)).astype(U64) & valid
    out = np.zeros((n, 2), U64)  # single bits, every entry in turn
    for i in range(n):
        k = i % max(nc, 1)
        if k < nc:
            out[i, k >> 6] = U64(1 << (k & 63))
    return out


@functools.lru_cache(maxsize=None)
def map_inputs(name, seed=1):
    """Every point family under every mask family, grouped: (points [n][3], masks [n][2], point family
    index [n], mask family index [n]), n ragged against 64.  The path family keeps its segments' own
    masks in the "logged" block."""
    sc = scene(name)
    fam = {"specials": specials(), "box": box_points(seed), "path": path_points(name)[0],
           "around": around_points(sc, seed + 1)[0], "cube": cube_points(sc, seed + 2)[0]}
    pts, masks, pf, mf = [], [], [], []
    for j, mname in enumerate(MASK_FAMILIES):
        for i, pname in enumerate(POINT_FAMILIES):
            p = fam[pname]
            # the specials go in as given; the rest keep to the range the oracle and the kernels share
            p = p if pname == "specials" else usable(p)
            m = mask_family(sc, mname, len(p), seed + 10 * i + j)
            if pname == "path" and mname == "logged":
                m = path_points(name)[1]
            pts.append(p), masks.append(m), pf.append(np.full(len(p), i)), mf.append(np.full(len(p), j))
    pts, masks, pf, mf = np.concatenate(pts), np.concatenate(masks), np.concatenate(pf), np.concatenate(mf)
    n = len(pts) - (len(pts) - 37) % 64 if len(pts) > 101 else len(pts)  # 64 k + 37
    for a in (pts, masks, pf, mf):
        a.setflags(write=False)
    return pts[:n], masks[:n], pf[:n], mf[:n]


def interleave(n, seed=5):
    """A permutation of the grouped order: position p takes the input whose rank of (67 i mod n, ties broken
    by a seeded jitter below 1/2) is p, so neighbouring lanes come from inputs about n / 67 apart in the
    grouped order and every wave mixes families, shapes and masks (test_map_ref.py counts the mixed waves)."""
    rng = np.random.default_rng(seed)
    order = np.argsort((np.arange(n) * 67) % n + rng.uniform(0, 0.5, n), kind="stable") if n > 1 else np.arange(n)
    return order


@functools.lru_cache(maxsize=None)
def map_expected(name, seed=1):
    """The oracle at map_inputs: (d, node); shared by the interpreter, table and baked kinds."""
    sc = scene(name)
    pts, masks = map_inputs(name, seed)[:2]
    d, node = sc.map(pts, masks)
    d.setflags(write=False), node.setflags(write=False)
    return d, node


# ---- hits, taps and their bounds -------------------------------------------------------
def tap_points(hits):
    """[n][6][3]: the six taps +x, -x, +y, -y, +z, -z at e = 1e-4, as meshref.normal forms them."""
    p = np.asarray(hits, F).reshape(-1, 3)
    e = F(0.0001)
    out = np.empty((len(p), 6, 3), F)
    for axis in range(3):
        for s, (on, off) in enumerate(((e, F(0.0)), (-e, F(-0.0)))):
            q = p + off
            q[:, axis] = p[:, axis] + on
            out[:, 2 * axis + s] = q
    return out


def tap_bound(d, q, t, bk):
    """pt_path.h tap_bound in float32 steps."""
    with np.errstate(all="ignore"):
        d, t, bk = np.asarray(d, F), np.asarray(t, F), F(bk)
        q = np.asarray(q, F).reshape(-1, 3)
        ad = np.abs(d)
        s = (((((np.abs(q[:, 0]) + np.abs(q[:, 1])).astype(F) + np.abs(q[:, 2])).astype(F) + ad).astype(F) +
              np.abs(t)).astype(F) + bk).astype(F)
        mg = (F(2.0 ** -10) * s).astype(F)
        return ((((d + ad).astype(F) * F(1.0 + 2.0 ** -16)).astype(F) + mg).astype(F) + F(float.fromhex("0x1.a38p-14"))).astype(F)


@functools.lru_cache(maxsize=None)
def hit_inputs(name, seed=3, max_hits=90, max_aimed=32):
    """Hit points of the logged rays, sphere-traced by the oracle to |F| < 1e-4 under the ray's mask, then
    of rays aimed at the shapes themselves under every check[] bit, each followed by the same point
    displaced by up to 2e-4; per hit its mask, the oracle's six tap
    values and nodes, and the four bounds.  A displaced point's pipeline bound is tap_bound of the march
    state (d = F(p), q = p, t): the bound's argument (3.13) holds for any state.  Hits with a non-finite
    tap value keep +inf in every bound family.  Dict of arrays."""
    sc = scene(name)
    rng = np.random.default_rng(seed)
    ro, rd, mask, _, _, hit = sc.segments
    hits, masks, qs, ds, ts = [], [], [], [], []
    with np.errstate(all="ignore"):
        for i in np.nonzero(hit)[0]:
            if len(hits) >= 2 * max_hits:
                break
            pts, dd, tt, ended = march(sc, ro[i], rd[i], mask[i], F(0.0001), steps=200)
            if not ended:
                continue
            h = (ro[i] + rd[i] * tt[-1]).astype(F)
            fh = sc.map(h, mask[i])[0][0]
            if not abs(fh) < 1e-4:
                continue
            hits.append(h), masks.append(mask[i]), qs.append(pts[-1]), ds.append(dd[-1]), ts.append(tt[-1])
            h2 = (h + rng.uniform(-2e-4, 2e-4, 3).astype(F)).astype(F)
            hits.append(h2), masks.append(mask[i]), qs.append(h2), ds.append(sc.map(h2, mask[i])[0][0]), ts.append(tt[-1])
        # and hits on the shapes themselves, which a 16 x 12 image need not see (tiny's specks lie behind
        # the camera): from 4 R out along a local direction towards each shape's origin, every check[] bit
        # set; at most max_aimed shapes, spread over the whole list
        ones = mask_family(sc, "ones", 1, 0)[0]
        shapes = [s for s in sc.shapes if np.isfinite(s["R"]) and s["R"] > 0 and np.isfinite(s["world"]) and s["world"] > 0]
        if len(shapes) > max_aimed:
            shapes = [shapes[i] for i in np.unique(np.round(np.linspace(0, len(shapes) - 1, max_aimed)).astype(int))]
        for s in shapes:
            v = rng.normal(size=3)
            o, c = to_world(s, 4.0 * s["R"] * v / np.linalg.norm(v))[0], to_world(s, np.zeros(3))[0]
            if not (np.isfinite(o).all() and np.abs(o).max() < 1e6 and np.linalg.norm(c - o) > 0):
                continue
            o, rd = o.astype(F), ((c - o) / np.linalg.norm(c - o)).astype(F)
            pts, dd, tt, ended = march(sc, o, rd, ones, F(0.0001), steps=200)
            if not ended:
                continue
            h = (o + rd * tt[-1]).astype(F)
            if not abs(sc.map(h, ones)[0][0]) < 1e-4:
                continue
            hits.append(h), masks.append(ones), qs.append(pts[-1]), ds.append(dd[-1]), ts.append(tt[-1])
            h2 = (h + rng.uniform(-2e-4, 2e-4, 3).astype(F)).astype(F)
            hits.append(h2), masks.append(ones), qs.append(h2), ds.append(sc.map(h2, ones)[0][0]), ts.append(tt[-1])
    hits = np.array(hits, F).reshape(-1, 3)
    masks = np.array(masks, U64).reshape(-1, 2)
    taps = tap_points(hits)
    d6, node6 = sc.map(taps.reshape(-1, 3), np.repeat(masks, 6, 0))
    d6, node6 = d6.reshape(-1, 6), node6.reshape(-1, 6)
    finite = np.isfinite(d6).all(1)
    inf = np.full(len(hits), np.inf, F)
    bounds = {"inf": inf, "nan": np.where(finite, F(np.nan), inf).astype(F),
              "pipeline": np.where(finite, tap_bound(np.array(ds, F), np.array(qs, F).reshape(-1, 3), np.array(ts, F),
                                                     sc.bound_k), inf).astype(F),
              "tightest": np.where(finite, d6.max(1, initial=-np.inf), inf).astype(F)}
    return dict(hits=hits, masks=masks, taps=taps, d6=d6, node6=node6, bounds=bounds, displaced=np.arange(len(hits)) % 2 == 1)


# ---- rays for bounds() -----------------------------------------------------------------
def _ulps(x, k):
    x = np.asarray(x, F).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
    return x


@functools.lru_cache(maxsize=None)
def ray_inputs(name, seed=7, max_boxes=12):
    """Rays for bounds(), grouped by family: (ro [n][3], rd [n][3], family index [n], family names).
    Logged segments; rays aimed at the corners and edge midpoints of the scene's own boxes (at most
    max_boxes of them, spread over the program's whole box list), exactly and a few ulps off (the
    undecided fallback); origins on box faces and inside boxes; axis-parallel
    directions and components below 2^-20 (outside the reciprocal guard)."""
    sc = scene(name)
    rng = np.random.default_rng(seed)
    lo, hi = sc.boxes
    ok = np.isfinite(lo).all(1) & np.isfinite(hi).all(1) & (np.abs(lo) < 1e6).all(1) & (np.abs(hi) < 1e6).all(1)
    lo, hi = lo[ok], hi[ok]
    if len(lo) > max_boxes:  # across the whole list: its first and last box, the mask words 2-3 included
        pick = np.unique(np.round(np.linspace(0, len(lo) - 1, max_boxes)).astype(int))
        lo, hi = lo[pick], hi[pick]
    fam, ros, rds = [], [], []

    def add(k, o, d):
        o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
        ros.append(o), rds.append(d), fam.append(np.full(len(o), k))

    sro, srd = sc.segments[:2]
    add(0, sro[:200], srd[:200])
    cam = np.array([0.0, 0.0, -3.0], F)
    for b in range(len(lo)):
        corners = np.array([[(lo[b], hi[b])[(c >> a) & 1][a] for a in range(3)] for c in range(8)], F)
        edges = np.array([(corners[i] + corners[j]) * F(0.5) for i in range(8) for j in range(i + 1, 8)
                          if bin(i ^ j).count("1") == 1], F)
        targets = np.concatenate([corners, edges])
        for origin in (cam, (cam + rng.uniform(-1, 1, 3)).astype(F)):
            d = (targets - origin).astype(F)
            for k in (0, 1, -2):
                add(1, np.repeat(origin[None], len(d), 0), _ulps(d, k) if k else d)
        # origins on a face (one coordinate exactly the box's) and inside
        for _ in range(4):
            o = (lo[b] + (hi[b] - lo[b]) * rng.uniform(0.05, 0.95, 3).astype(F)).astype(F)
            face = o.copy()
            a = rng.integers(3)
            face[a] = (lo[b], hi[b])[rng.integers(2)][a]
            d = rng.normal(size=(2, 3)).astype(F)
            add(2, [face, o], d)
    axes = np.array([(0, 0, 1), (1, 0, 0), (0, -1, 0), (-0.0, 0.0, 1.0), (1e-7, 1.0, 3e-8), (1.0, -2e-7, 1e-9),
                     (0.0, 1e-30, 1.0), (1e-7, 1e-7, 1e-7)], F)
    for d in axes:
        o = rng.uniform(-2, 2, (6, 3)).astype(F)
        o[:, 2] -= F(2.0)
        add(3, o, np.repeat(d[None], len(o), 0))
    ro, rd, fam = np.concatenate(ros), np.concatenate(rds), np.concatenate(fam)
    n = len(ro) - (len(ro) - 37) % 64 if len(ro) > 101 else len(ro)
    return ro[:n], rd[:n], fam[:n], ("logged", "corners and edges", "faces and insides", "axis-parallel and tiny")


@functools.lru_cache(maxsize=None)
def skip_rays(name, seed=9, waves=10):
    """Rays for skip_mode 1, by wave of 64: full waves of jittered directions from one origin (the first
    pass's windows: the camera's, towards each image region and towards box corners), waves with two
    origins, and a ragged last wave.  (ro, rd)."""
    sc = scene(name)
    rng = np.random.default_rng(seed)
    lo, hi = sc.boxes
    cam = np.array([0.0, 0.0, -3.0], F)
    ros, rds = [], []
    for w in range(waves):
        if w % 2 == 0 or not len(lo):
            centre = np.array([rng.uniform(-1.3, 1.3), rng.uniform(-1, 1), 1.0])
        else:
            b = rng.integers(len(lo))
            centre = np.where(rng.integers(2, size=3), hi[b], lo[b]).astype(np.float64) - cam
            if not np.isfinite(centre).all() or np.abs(centre).max() > 1e6:
                centre = np.array([0.1, 0.1, 1.0])
        d = centre + rng.uniform(-1, 1, (64, 3)) * (0.002 if w % 3 else 0.05)
        d /= np.linalg.norm(d, axis=1)[:, None]
        o = np.repeat(cam[None], 64, 0)
        if w in (3, 7):  # two origins in one wave
            o[32:] = (cam + np.array([0.25, -0.1, 0.0])).astype(F)
        ros.append(o), rds.append(d.astype(F))
    ro, rd = np.concatenate(ros), np.concatenate(rds)
    return ro[:len(ro) - 27], rd[:len(rd) - 27]  # (the last wave ragged: 37 rays)


def albedo_of_nodes(sc, node):
    return meshref.node_albedo(sc.rows, node)


def albedo_of_shapes(sc, shape, data=None):
    """The albedo of the product's shape ordinals (Hit.m - 1), as Mesh.vertex_colors reads it."""
    from compute_path_tracer_amd.path_tracer import Mesh

    s = np.asarray(shape, np.int32).reshape(-1)
    return Mesh(np.zeros((len(s), 3), F), np.zeros((len(s), 3), F), s, np.zeros((0, 3))).vertex_colors(sc.prog, data)
