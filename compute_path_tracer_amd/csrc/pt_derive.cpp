// pt_derive.cpp -- host-only scene derivation: the expansion of (program,
// data[]) into the device tables (pt_device.h) and the bounds the scene
// kernels cull by.  Shared by pt_runtime.hip (pt_set_data) and pt_jit.cpp.
// Every value is the f32 expression the generated GLSL evaluates on the GPU,
// evaluated here once with the same rounding (see pt_device.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/pt_abi.h"
#include "pt_device.h"
#include "pt_host.h"
#include "pt_math.h"

// Distance-bound culling data for the scene kernels (pt_jit.cpp, DESIGN.md
// 3.12), in PtNode.pad[0]:
//  * shape: R' = R + 2^-12 (|R| + |m|_1), where R bounds the shape from its
//    local origin (sdf(q) >= |q| - R: sphere r, cube |b|, torus |R1| + r,
//    octahedron s), or NaN when the node's values are outside the range the
//    rounding argument covers (never culled);
//  * union begin: the matching end's 1/s when the union may drop shapes that
//    cannot beat its parent's running distance (it combines into the parent by
//    union, has no child unions, only assign/union shapes, all with finite
//    R'), else NaN.
void pt_cull_bounds(std::vector<PtNode> &nodes) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const double big = 1099511627776.0;  // 2^40
    auto fin = [&](float v) { return std::isfinite(v) && std::fabs(double(v)) <= big; };
    for (PtNode &d : nodes) {
        d.pad[0] = nan;
        if (d.op != PT_OP_SHAPE) continue;
        bool ok = std::isfinite(d.inv) && d.inv >= 0x1p-20f && d.inv <= 0x1p20f && fin(d.m[0]) && fin(d.m[1]) &&
                  fin(d.m[2]) && fin(d.cx) && fin(d.sx) && fin(d.cy) && fin(d.sy) && fin(d.cz) && fin(d.sz);
        double R = 0.0;
        switch (d.shape) {
            case PT_NODE_SPHERE: ok = ok && fin(d.size[0]); R = d.size[0]; break;
            case PT_NODE_CUBE:
                ok = ok && fin(d.size[0]) && fin(d.size[1]) && fin(d.size[2]) && d.size[0] >= 0.0f &&
                     d.size[1] >= 0.0f && d.size[2] >= 0.0f;
                R = std::sqrt(double(d.size[0]) * d.size[0] + double(d.size[1]) * d.size[1] +
                              double(d.size[2]) * d.size[2]);
                break;
            case PT_NODE_TORUS:
                ok = ok && fin(d.size[0]) && fin(d.size[1]);
                R = std::fabs(double(d.size[0])) + double(d.size[1]);
                break;
            case PT_NODE_OCTAHEDRON: ok = ok && fin(d.size[0]) && d.size[0] >= 0.0f; R = d.size[0]; break;
            default: ok = false;
        }
        if (!ok) continue;
        const double m1 = std::fabs(double(d.m[0])) + std::fabs(double(d.m[1])) + std::fabs(double(d.m[2]));
        d.pad[0] = float(R + 0x1p-12 * (std::fabs(R) + m1));
    }
    for (size_t i = 0; i < nodes.size(); ++i) {
        if (nodes[i].op != PT_OP_UNION_BEGIN) continue;
        size_t j = i + 1;
        bool ok = true;
        for (; j < nodes.size() && nodes[j].op != PT_OP_UNION_END; ++j) {
            const PtNode &c = nodes[j];
            if (c.op != PT_OP_SHAPE || !(c.combine == PT_COMBINE_ASSIGN || c.combine == PT_COMBINE_UNION) ||
                !std::isfinite(c.pad[0]))
                ok = false;  // a child union, a subtraction, or a shape without a bound
        }
        if (j == nodes.size()) continue;
        const PtNode &e = nodes[j];
        ok = ok && e.combine == PT_COMBINE_UNION && std::isfinite(e.inv) && e.inv > 0.0f;
        if (ok) nodes[i].pad[0] = e.inv;
    }
}

// Margin constant of the map() bound (pt_path.h tap_bound):
// the largest transform-chain magnitude of any shape in world units -- the
// |pos| of every enclosing union and of the shape, plus the shape's radius
// bound R, each in world units.  The rounding error of a map() evaluation at
// q is a few tens of ulp of |q|_1 + K; the kernels' margin is 2^-10 times
// that.  NaN (no bound) when any 1/s is outside [1/2, 2] or any value is
// beyond 2^20.
float pt_bound_k(const std::vector<PtNode> &nodes) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    auto fin = [](double v) { return std::isfinite(v) && std::fabs(v) <= 1048576.0; };
    double K = 0.0;
    std::vector<double> scale(1, 1.0), reach(1, 0.0);  // world units per local unit; |pos| chain so far
    for (const PtNode &d : nodes) {
        if (d.op == PT_OP_UNION_END) {
            if (scale.size() > 1) {
                scale.pop_back();
                reach.pop_back();
            }
            continue;
        }
        if (!(std::isfinite(d.inv) && d.inv >= 0.5f && d.inv <= 2.0f)) return nan;
        for (float v : {d.m[0], d.m[1], d.m[2], d.size[0], d.size[1], d.size[2]})
            if (!fin(v)) return nan;
        const double sc = scale.back() / double(d.inv);  // this node's local unit in world units
        const double r = reach.back() + (std::fabs(double(d.m[0])) + std::fabs(double(d.m[1])) +
                                         std::fabs(double(d.m[2]))) * sc;
        if (d.op == PT_OP_UNION_BEGIN) {
            scale.push_back(sc);
            reach.push_back(r);
            continue;
        }
        double R;
        switch (d.shape) {
            case PT_NODE_SPHERE: R = std::fabs(double(d.size[0])); break;
            case PT_NODE_CUBE:
                R = std::sqrt(double(d.size[0]) * d.size[0] + double(d.size[1]) * d.size[1] +
                              double(d.size[2]) * d.size[2]);
                break;
            case PT_NODE_TORUS: R = std::fabs(double(d.size[0])) + std::fabs(double(d.size[1])); break;
            case PT_NODE_OCTAHEDRON: R = std::fabs(double(d.size[0])); break;
            default: return nan;
        }
        K = std::max(K, r + R * sc);
    }
    return float(K * (1.0 + 0x1p-20));
}

bool pt_fast_bounds(const std::vector<PtAabb> &boxes) {
    for (const PtAabb &b : boxes)
        for (int k = 0; k < 3; ++k)
            if (!pt_div_coord_ok(b.bmin[k]) || !pt_div_coord_ok(b.bmax[k])) return false;
    return true;
}

int pt_derive(const std::vector<pt_op> &ops, const std::vector<pt_aabb> &aabbs, const float *data, uint32_t n,
              std::vector<PtNode> &nodes, std::vector<PtAabb> &boxes, std::vector<PtMat> &mats, std::string &err) {
    auto bad = [&](const char *msg) {
        err = msg;
        return PT_ERR_INVALID;
    };
    auto in = [&](uint32_t s) { return s < n; };
    nodes.resize(ops.size());
    mats.clear();
    PtMat mdef;
    std::memset(&mdef, 0, sizeof mdef);
    {
        pt_f3 z{0.0f, 0.0f, 0.0f};
        pt_f3 nl = pt_normalize(z);  // MDEF light = vec3(0): normalize -> NaN, as upstream
        mdef.emis[0] = nl.x * 0.0f;
        mdef.emis[1] = nl.y * 0.0f;
        mdef.emis[2] = nl.z * 0.0f;
    }
    mats.push_back(mdef);
    for (size_t i = 0; i < ops.size(); ++i) {
        const pt_op &op = ops[i];
        PtNode &d = nodes[i];
        std::memset(&d, 0, sizeof d);
        d.op = int32_t(op.opcode);
        d.shape = int32_t(op.shape);
        d.combine = int32_t(op.combine);
        d.check = op.check;
        if (!in(op.scale)) return bad("op references data slot out of range");
        for (int k = 0; k < 3; ++k)
            if (!in(op.position[k]) || !in(op.rotation[k]))
                return bad("op references data slot out of range");
        const float s = data[op.scale];
        const float inv = 1.0f / s;  // `1.0 / data[scale]`
        d.inv = inv;
        for (int k = 0; k < 3; ++k) d.m[k] = data[op.position[k]] * inv;  // pos * (1.0 / s)
        pt_sincos(data[op.rotation[0]], d.sx, d.cx);
        pt_sincos(data[op.rotation[1]], d.sy, d.cy);
        pt_sincos(data[op.rotation[2]], d.sz, d.cz);
        // The reference multiplies by three full matrices (shapes.glsl:34-68),
        // zeros included, and 0 * NaN = 0 * inf = NaN: one non-finite
        // coordinate after the translation, or a NaN rotation about x or y,
        // leaves all three coordinates NaN after the third matrix.  xform_f
        // skips the zero terms, so it would keep the untouched coordinates
        // finite.  A NaN translation makes them all NaN at once instead.  A
        // NaN rotation about z, the last matrix, leaves a shape's z alone in
        // both; a union hands (NaN, NaN, z) on to its children, whose own
        // full matrices make z NaN too, so for a union it counts as well.
        const bool z_nan = op.opcode == PT_OP_UNION_BEGIN && (!std::isfinite(d.sz) || !std::isfinite(d.cz));
        if (!std::isfinite(inv) || !std::isfinite(d.m[0]) || !std::isfinite(d.m[1]) || !std::isfinite(d.m[2]) ||
            !std::isfinite(d.sx) || !std::isfinite(d.cx) || !std::isfinite(d.sy) || !std::isfinite(d.cy) || z_nan)
            d.m[0] = d.m[1] = d.m[2] = std::numeric_limits<float>::quiet_NaN();
        uint32_t f = 0;
        if (inv != 1.0f) f |= PT_NF_SCALE;
        if (d.m[0] != 0.0f || d.m[1] != 0.0f || d.m[2] != 0.0f) f |= PT_NF_POS;
        if (!(d.cx == 1.0f && d.sx == 0.0f)) f |= PT_NF_RX;
        if (!(d.cy == 1.0f && d.sy == 0.0f)) f |= PT_NF_RY;
        if (!(d.cz == 1.0f && d.sz == 0.0f)) f |= PT_NF_RZ;
        d.flags = f;
        if (op.opcode == PT_OP_SHAPE) {
            for (int k = 0; k < 3; ++k) {
                if (!in(op.size[k])) return bad("size slot out of range");
                d.size[k] = data[op.size[k]];
            }
            for (int k = 0; k < 18; ++k)
                if (!in(op.material[k])) return bad("material slot out of range");
            const uint32_t *ms = op.material;
            PtMat m;
            std::memset(&m, 0, sizeof m);
            for (int k = 0; k < 3; ++k) {
                m.col[k] = data[ms[k]];
                m.spec_col[k] = data[ms[8 + k]];
            }
            m.spec = data[ms[7]];
            m.rough2 = data[ms[11]] * data[ms[11]];
            pt_f3 nl = pt_normalize(pt_f3{data[ms[4]], data[ms[5]], data[ms[6]]});
            const float br = data[ms[3]];
            m.emis[0] = nl.x * br;
            m.emis[1] = nl.y * br;
            m.emis[2] = nl.z * br;
            d.mat = int32_t(mats.size());
            mats.push_back(m);
        }
    }
    pt_cull_bounds(nodes);
    boxes.resize(aabbs.size());
    for (size_t i = 0; i < aabbs.size(); ++i) {
        const pt_aabb &a = aabbs[i];
        for (int k = 0; k < 3; ++k)
            if (!in(a.union_position[k]) || !in(a.shape_position[k]) || !in(a.size[k]))
                return bad("aabb slot out of range");
        if (!in(a.union_scale) || !in(a.shape_scale) || !in(a.aabb_exaggeration))
            return bad("aabb slot out of range");
        float so[3];
        switch (a.so_kind) {
            case PT_SO_SCALAR: so[0] = so[1] = so[2] = data[a.size[0]]; break;
            case PT_SO_VEC3:
                for (int k = 0; k < 3; ++k) so[k] = data[a.size[k]];
                break;
            case PT_SO_TORUS: {
                const float R = data[a.size[0]], r = data[a.size[1]];
                so[0] = R + r;
                so[1] = r;
                so[2] = R + r;
                break;
            }
            default: so[0] = so[1] = so[2] = 1.0f; break;
        }
        const float sc = data[a.union_scale] * data[a.shape_scale];
        const float ex = data[a.aabb_exaggeration];
        PtAabb &b = boxes[i];
        std::memset(&b, 0, sizeof b);
        for (int k = 0; k < 3; ++k) {
            const float ctr = data[a.union_position[k]] + data[a.shape_position[k]];
            const float hs = (so[k] * sc) * ex;
            b.bmin[k] = ctr - hs;  // from_pos_size (aabb.glsl:13-19)
            b.bmax[k] = ctr + hs;
        }
        b.back = a.back;
    }
    return PT_OK;
}
