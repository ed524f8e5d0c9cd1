// pt_jit.cpp -- per-scene specialisation of map(): the source generator.
//
// The reference turns the editor tree into GLSL text and recompiles its
// compute shader whenever the topology changes (SDFEditor::compile,
// sdf_editor.rs:186-246 -> PathTracer::remake_pipeline, path_tracer.rs:62-95),
// while value edits only refresh data[].  This file does the same for the
// HIP kernel: the op list becomes straight-line device code (one block per
// union/shape, exactly the statement order of the generated GLSL), with each
// node's shape kind, combine op and identity-elision flags as template
// arguments, while every float value is still read from the node table, so
// value-only edits keep the compiled kernel (unless an identity flag flips).
// Host only: pt_jit_build.cpp compiles the text with hipRTC, pt_jit_state.cpp
// loads and selects the kernels.
//
// pt_jit_source is the driver: analyse() once (what each node and union is,
// independent of the map variant), then one MapEmitter per variant (JitMap,
// JitMapB0, JitMapB1: DESIGN.md 3.12 / 3.13), then the scene's bounds(),
// traits, wave macros and kernel entry points.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

#include "pt_host.h"

namespace {

// ---- analysis: what every node is, whichever map variant is emitted -----------------

struct NodeInfo {
    float wscale = 1.0f;  // world scale: the node's own scale times its enclosing unions'
    // UNION_BEGIN.  parent_rule: its shapes may be dropped against the parent's
    // running distance -- it unions into the parent, has no child unions, only
    // assign/union shapes (pt_cull_bounds checks the values: NaN in pad[0]
    // switches it off).  later_union, top level only: every later top-level
    // combine is a union, so the map() bound rule may apply.
    bool parent_rule = false, later_union = false;
    // bound-culled unions (top level, later_union, parent rule; whole unions,
    // up to 64 shapes in all): a shape's bit in `live`, its union's mask of them
    int live_bit = -1;
    uint64_t live_mask = 0;
    // UNION_BEGIN: the matching UNION_END; flat: its children are shapes only,
    // at least one; their check[] bits below 64, and whether that is all of them
    size_t end = 0;
    bool flat = false, check_narrow = false;
    uint64_t check_mask = 0;
};

std::vector<NodeInfo> analyse(const std::vector<PtNode> &nodes) {
    const size_t n = nodes.size();
    std::vector<NodeInfo> info(n);
    struct Open {
        size_t begin;
        float scale;
        bool shapes_only = true, assign_union_only = true, narrow = true;
        int shapes = 0;
    };
    std::vector<Open> open;
    std::vector<std::pair<size_t, int>> top;  // (BEGIN index or n, combine) of the top-level combines in order
    for (size_t i = 0; i < n; ++i) {
        const PtNode &d = nodes[i];
        const float s = (std::isfinite(d.inv) && d.inv != 0.0f) ? 1.0f / d.inv : 1.0f;
        const float outer = open.empty() ? 1.0f : open.back().scale;
        if (d.op == PT_OP_UNION_BEGIN) {
            if (!open.empty()) open.back().shapes_only = false;
            info[i].end = n;
            info[i].wscale = outer * s;
            open.push_back(Open{i, outer * s});
        } else if (d.op == PT_OP_UNION_END) {
            if (open.empty()) break;
            const Open u = open.back();
            open.pop_back();
            NodeInfo &b = info[u.begin];
            b.end = i;
            b.flat = u.shapes_only && u.shapes > 0;
            b.check_narrow = u.narrow;
            b.parent_rule = u.shapes_only && u.assign_union_only && d.combine == PT_COMBINE_UNION;
            if (open.empty()) top.push_back({u.begin, d.combine});
        } else {
            info[i].wscale = outer * s;
            if (open.empty()) {
                top.push_back({n, d.combine});
                continue;
            }
            Open &u = open.back();
            u.shapes += 1;
            if (d.op != PT_OP_SHAPE || !(d.combine == PT_COMBINE_ASSIGN || d.combine == PT_COMBINE_UNION))
                u.assign_union_only = false;
            if (d.check >= 0 && d.check < 64) info[u.begin].check_mask |= 1ull << d.check;
            else u.narrow = false;
        }
    }
    bool all_union = true;  // every top-level combine after this one is a union
    for (size_t k = top.size(); k-- > 0;) {
        if (top[k].first < n) info[top[k].first].later_union = all_union;
        all_union = all_union && top[k].second == PT_COMBINE_UNION;
    }
    int nbits = 0;
    for (const auto &t : top) {
        if (t.first == n || !(info[t.first].parent_rule && info[t.first].later_union)) continue;
        const int cnt = int(info[t.first].end - t.first - 1);
        if (nbits + cnt > 64) continue;
        for (int k = 0; k < cnt; ++k) {
            info[t.first + 1 + size_t(k)].live_bit = nbits + k;
            info[t.first].live_mask |= 1ull << (nbits + k);
        }
        nbits += cnt;
    }
    return info;
}

// ---- text fragments -----------------------------------------------------------------

// exact f32 literal (hex float) for baked constants
std::string hexf(float v) {
    char buf[64];
    if (v != v) return "__builtin_nanf(\"\")";
    if (v == __builtin_inff()) return "__builtin_inff()";
    if (v == -__builtin_inff()) return "(-__builtin_inff())";
    std::snprintf(buf, sizeof buf, "%af", double(v));
    return buf;
}

// an integer mask as a hex literal: hex_lit(m, "ull"), hex_lit(w, "u")
std::string hex_lit(uint64_t v, const char *suffix) {
    char buf[32];
    std::snprintf(buf, sizeof buf, "0x%llx%s", static_cast<unsigned long long>(v), suffix);
    return buf;
}

// X widened by the cull tests' rounding margin: X + 2^-12 |X|
std::string margin(const std::string &x) { return "__builtin_fmaf(fabsf(" + x + "), 0x1p-12f, " + x + ")"; }

std::string baked_node(const PtNode &n, size_t i) {
    std::ostringstream o;
    o << "    constexpr PtNode B" << i << "{" << n.op << ", " << n.shape << ", " << n.combine << ", " << n.check << ", "
      << n.mat << ", " << n.flags << "u, " << hexf(n.inv) << ", {" << hexf(n.m[0]) << ", " << hexf(n.m[1]) << ", "
      << hexf(n.m[2]) << "}, " << hexf(n.cx) << ", " << hexf(n.sx) << ", " << hexf(n.cy) << ", " << hexf(n.sy) << ", "
      << hexf(n.cz) << ", " << hexf(n.sz) << ", {" << hexf(n.size[0]) << ", " << hexf(n.size[1]) << ", "
      << hexf(n.size[2]) << "}, {" << hexf(n.pad[0]) << ", 0, 0, 0, 0}};\n";
    return o.str();
}

// cubes whose SDF takes cube_from_q's one-face path: a
// middle half-extent >= 1 in world units (C3's walls, floor, roof, light;
// every cube measured equal, none -1.2 %)
bool fast_cube(const PtNode &n, float world_scale) {
    if (n.shape != PT_NODE_CUBE) return false;
    float b[3] = {std::fabs(n.size[0]), std::fabs(n.size[1]), std::fabs(n.size[2])};
    std::sort(b, b + 3);
    return b[1] * world_scale >= 1.0f;
}

// the lane's own check[] bit k
std::string lane_bit(int k) {
    return std::string(k < 64 ? "((ck.lo >> " : "((ck.hi >> ") + std::to_string(k < 64 ? k : k - 64) + ") & 1ull)";
}

// a shape's check[] test as a condition (a shape without a box always runs)
std::string check_test(const PtNode &n) { return n.check >= 0 ? lane_bit(n.check) : "true"; }

// bit k of a wave-uniform 128-bit mask (ck.alo, ck.ahi) as a 32-bit test on
// the words guard_words() makes opaque scalars: LLVM folds `s_and_b32` +
// compare into one bit test and branch (2 SALU), where a 64-bit test kept
// `s_and_b32, s_cmp_eq_u64, s_cbranch` (and InstCombine turns a test of a
// truncated word back into the 64-bit one)
std::string wave_bit(int k) {
    const int b = k & 63;
    return std::string("((") + (k < 64 ? "cka" : "ckh") + (b >= 32 ? "1" : "0") + " >> " + std::to_string(b & 31) +
           ") & 1u)";
}

// the preamble for wave_bit(): ck.alo / ck.ahi as four 32-bit scalars
const char *guard_words() {
    return "    const uint32_t cka0 = __builtin_amdgcn_readfirstlane(uint32_t(ck.alo)),\n"
           "                   cka1 = __builtin_amdgcn_readfirstlane(uint32_t(ck.alo >> 32)),\n"
           "                   ckh0 = __builtin_amdgcn_readfirstlane(uint32_t(ck.ahi)),\n"
           "                   ckh1 = __builtin_amdgcn_readfirstlane(uint32_t(ck.ahi >> 32));\n"
           "    (void)cka0; (void)cka1; (void)ckh0; (void)ckh1;\n";
}

// The guard in front of a shape with a box, `if (lane) ` or `if (wave) if
// (lane) `: check[] bit k of the wave's union of masks (ck.alo / ck.ahi,
// wave-uniform: a scalar bit test and branch) before the lane's own bit, so a
// shape no lane of the wave needs costs no vector instructions (JitMap only,
// the trace pass; in the shade pass's taps the extra blocks cost the kernel
// 40 spilled VGPRs at its 72-register budget)
std::string check_guard(const PtNode &n, bool wave) {
    const int k = n.check;
    if (k < 0) return "";
    if (!wave) return "if (" + lane_bit(k) + ") ";
    return "if (" + wave_bit(k) + ") if (lane_check(" + (k < 64 ? "ck.lo, " : "ck.hi, ") +
           std::to_string(k < 64 ? k : k - 64) + ")) ";
}

std::string count_shape(const PtNode &n) {
    return "count_shape(st, " + std::to_string(n.shape) + ", " + std::to_string(n.combine) + ")";
}
// a dropped shape still counts (algorithmic work = the oracle's), as culled
std::string count_culled(const PtNode &n) { return "{ " + count_shape(n) + "; st.add(PT_ST_CULLED); }"; }

// A dropped first (assign) shape stands in as +inf, not MAXHIT: the
// reference's u = shape overwrites MAXHIT (containers.rs:244-252), and its
// value is > the target
std::string drop_assign(const std::string &D, const PtNode &n) {
    return "h" + D + " = Hit{__builtin_inff(), " + std::to_string(n.mat) + "};";
}

// what an empty union hands its parent: its MAXHIT start divided by its scale
float scaled_by_end(float v, const PtNode &end) { return (end.flags & PT_NF_SCALE) ? v / end.inv : v; }

// ---- one map() variant --------------------------------------------------------------

// JitMap: march steps and in-trace normal taps.  JitMapB0 / JitMapB1: the
// same map() plus the bound rule, for the shade pass's normal taps
// (DESIGN.md 3.13).  B0 (first tap) also records in `live` which shapes
// of the bound-culled unions may matter at any of the six taps (its test
// against the widened bound bndw); B1 (the other five) evaluates exactly
// those, without tests.
struct MapVariant {
    const char *name;
    // map() bound rule: a top-level union whose later
    // top-level combines are all unions may also drop shapes whose distance
    // provably exceeds the lane's bound on the final map() value (eval's bnd).
    // That gives the first union (parent still MAXHIT) a target.  Without it
    // (the trace map) the cull tests take the forms tuned for the march loop.
    bool bound_rule;
    bool records_live, uses_live;
    bool wave_guards;  // check[] tests look at the wave's union of masks first (check_guard)
};
constexpr MapVariant kMapVariants[] = {{"JitMap", false, false, false, true},
                                       {"JitMapB0", true, true, false, false},
                                       {"JitMapB1", true, false, true, false}};

// an open union while its body is emitted (the bottom frame: the top level, h0)
struct OpenUnion {
    size_t begin = 0;
    int depth = 0;
    bool masked = false;   // B1 wrapped its body in a live-mask test
    bool skipped = false;  // its body sits in the else of a "no lane needs it" shortcut
    bool cull_on = false;  // its shapes carry cull tests (or, masked, live-bit tests)
    bool use_bnd = false;  // ... whose target includes the map() bound
    // A union whose parent accumulator still holds its MAXHIT start value
    // (nothing combined into it yet, e.g. the first top-level union) has
    // nothing to cull against: its cull tests would never fire, so it gets
    // none (+4 %) unless the bound rule gives it a target.
    bool parent_fresh = false;
    bool fresh = true;  // its own accumulator is still MAXHIT
};

class MapEmitter {
  public:
    MapEmitter(std::ostringstream &out, const std::vector<PtNode> &nodes, const std::vector<NodeInfo> &info, bool bake,
               const MapVariant &v)
        : o(out), nodes(nodes), info(info), bake(bake), v(v) {}

    void emit() {
        o << "struct " << v.name << " {\n"
             "  template <bool ST>\n"
             "  static __device__ __forceinline__ Hit eval(const PtLaunch &L, float qx, float qy, float qz,\n"
             "                                             const Check &ck, float bnd, float bndw, uint64_t &live,\n"
             "                                             Stats<ST> &st) {\n"
             "    (void)bnd;\n"
             "    (void)bndw;\n"
             "    (void)live;\n"
             "    const cnode_ptr N = (cnode_ptr)L.nodes;\n"
             "    (void)N;\n"
             "    Hit h0{kMaxHit, 0};\n"
             "    const float x0 = qx, y0 = qy, z0 = qz;\n";
        o << guard_words();
        if (bake)  // values as exact literals: no scalar loads, constant folding
            for (size_t i = 0; i < nodes.size(); ++i) o << baked_node(nodes[i], i);
        open.assign(1, OpenUnion{});
        for (size_t i = 0; i < nodes.size(); ++i) {
            if (nodes[i].op == PT_OP_UNION_BEGIN) union_begin(i);
            else if (nodes[i].op == PT_OP_SHAPE) shape(i);
            else if (open.size() > 1) union_end(i);
        }
        o << "    return h0;\n"
             "  }\n"
             "};\n";
    }

  private:
    std::ostringstream &o;
    const std::vector<PtNode> &nodes;
    const std::vector<NodeInfo> &info;
    const bool bake;
    const MapVariant &v;
    std::vector<OpenUnion> open;

    std::string ref(size_t i) const { return bake ? "B" + std::to_string(i) : "N[" + std::to_string(i) + "]"; }
    std::string times_inv(size_t i) const { return (nodes[i].flags & PT_NF_SCALE) ? " * " + ref(i) + ".inv" : ""; }
    bool one_face(size_t i) const { return fast_cube(nodes[i], info[i].wscale); }
    std::string sdf_call(size_t i) const {
        return "sdf_k<" + std::to_string(nodes[i].shape) + (one_face(i) ? ", true" : "") + ">(" + ref(i) + ", x, y, z)";
    }
    std::string cube_from_q(size_t i) const {
        return std::string("cube_from_q<") + (one_face(i) ? "true" : "false") + ">(qx, qy, qz, qm)";
    }

    // `d = d / inv` of a scaled node: in the baked build by the constant's
    // correctly rounded reciprocal (pt_div_k; |inv| in [2^-4, 2^4]: every map
    // variant), else the IEEE division
    void divide(const char *in, size_t i) {
        if (!(nodes[i].flags & PT_NF_SCALE)) return;
        const float b = nodes[i].inv, ab = std::fabs(b);
        if (!bake || !(ab >= 0x1p-4f && ab <= 0x1p4f)) o << in << "d = d / " << ref(i) << ".inv;\n";
        else o << in << "d = pt_div_k(d, " << ref(i) << ".inv, " << hexf(1.0f / b) << ");\n";
    }
    // the end of every shape: its distance d, unscaled, joins the union's accumulator
    void shape_tail(const char *in, size_t i, const std::string &D) {
        divide(in, i);
        const PtNode &n = nodes[i];
        o << in << "h" << D << " = combine_c<" << n.combine << ">(h" << D << ", Hit{d, " << n.mat << "});\n";
    }
    // a union's value (or its stand-in) joins the parent's accumulator
    void combine_parent(const char *in, const PtNode &end, const std::string &P, const std::string &hit) {
        o << in << "h" << P << " = combine_c<" << end.combine << ">(h" << P << ", " << hit << ");\n"
          << in << "st.add(" << (end.combine == PT_COMBINE_UNION ? "PT_ST_COMB_UNION" : "PT_ST_COMB_SUB") << ");\n";
    }
    // a cube's per-axis distances and their maximum: sdCube >= max(q) in f32 for
    // max(q) > 2^-60 (below it RN(qm^2) may underflow)
    void cube_q(const char *in, size_t i) {
        o << in << "const float qx = fabsf(x) - " << ref(i) << ".size[0], qy = fabsf(y) - " << ref(i)
          << ".size[1], qz = fabsf(z) - " << ref(i) << ".size[2];\n"
          << in << "const float qm = pt_gmax(qx, pt_gmax(qy, qz));\n";
    }
    // a shape's block opens: its check[] guard, the union's point, transform part `flags`
    void shape_open(size_t i, const std::string &D, uint32_t flags) {
        o << "    " << check_guard(nodes[i], v.wave_guards) << "{  // shape " << i << "\n"
          << "      float x = x" << D << ", y = y" << D << ", z = z" << D << ";\n"
          << "      xform_f<" << flags << "u>(" << ref(i) << ", x, y, z);\n";
    }

    void union_begin(size_t i) {
        const NodeInfo &a = info[i];
        const OpenUnion par = open.back();
        OpenUnion u;
        u.begin = i;
        u.depth = par.depth + 1;
        const std::string D = std::to_string(u.depth), P = std::to_string(par.depth);
        u.masked = v.uses_live && a.live_mask != 0;
        o << "    {  // union " << i << "\n"
          << "    Hit h" << D << "{kMaxHit, 0};\n"
          << "    st.add(PT_ST_XFORM_UNION);\n";
        if (u.masked && a.flat) shortcut_no_live(i, P);
        else if (a.flat && a.check_narrow) shortcut_no_check(i, P);
        u.skipped = a.flat && (u.masked || a.check_narrow);
        if (u.masked) o << "    if ((live & " << hex_lit(a.live_mask, "ull") << ") != 0ull) {\n";
        o << "    float x" << D << " = x" << P << ", y" << D << " = y" << P << ", z" << D << " = z" << P << ";\n"
          << "    xform_f<" << nodes[i].flags << "u>(" << ref(i) << ", x" << D << ", y" << D << ", z" << D << ");\n";
        u.use_bnd = v.bound_rule && par.depth == 0 && a.later_union;
        u.parent_fresh = par.fresh;
        u.cull_on = a.parent_rule && (!par.fresh || u.use_bnd);
        if (u.cull_on && !u.masked) cull_targets(i, u, P);
        open.push_back(u);
    }

    // taps 2-6 (B1): a bound-culled union none of whose shapes is live in any
    // active lane gives each lane its first shape's +inf stand-in (check[]
    // admits it) or MAXHIT, divided by the union's scale on the host (+inf /
    // inv, 10000 / inv)
    void shortcut_no_live(size_t i, const std::string &P) {
        const PtNode &end = nodes[info[i].end];
        const std::string inf = hexf(scaled_by_end(__builtin_inff(), end));
        o << "    if (__ballot((live & " << hex_lit(info[i].live_mask, "ull") << ") != 0ull) == 0ull) {\n"
          << "      Hit hu{" << hexf(scaled_by_end(10000.0f, end)) << ", 0};\n";
        for (size_t j = i + 1; j < info[i].end; ++j) {
            const PtNode &c = nodes[j];
            if (c.combine == PT_COMBINE_ASSIGN)
                o << "      if (" << check_test(c) << ") hu = Hit{" << inf << ", " << c.mat << "};\n";
            o << "      if constexpr (ST) {\n"
              << "        if (" << check_test(c) << ") " << count_culled(c) << "\n"
              << "      }\n";
        }
        combine_parent("      ", end, P, "hu");
        o << "    } else {\n";
    }

    // A union whose shapes no lane needs returns its MAXHIT start, i.e. the
    // constant kMaxHit / inv with material 0, to its parent -- without its
    // transform, bound setup and division.  Trace: the wave's union of check[]
    // masks ck.alo, a scalar test; the shade pass's taps: a ballot of the
    // active lanes' own check[] bits.
    void shortcut_no_check(size_t i, const std::string &P) {
        const PtNode &end = nodes[info[i].end];
        const uint64_t m = info[i].check_mask;
        if (!v.wave_guards) o << "    if (__ballot((ck.lo & " << hex_lit(m, "ull") << ") != 0ull) == 0ull) {\n";
        else if ((m >> 32) == 0) o << "    if ((cka0 & " << hex_lit(m, "u") << ") == 0u) {\n";
        else if ((m & 0xffffffffull) == 0) o << "    if ((cka1 & " << hex_lit(m >> 32, "u") << ") == 0u) {\n";
        else o << "    if ((ck.alo & " << hex_lit(m, "ull") << ") == 0ull) {\n";
        combine_parent("      ", end, P, "Hit{" + hexf(scaled_by_end(10000.0f, end)) + ", 0}");
        o << "    } else {\n";
    }

    // What a culling union's shapes test against.  The rounding argument needs
    // a bounded point (pb); tg: the parent's running distance (or the map()
    // bound when smaller) in this union's frame (NaN: rule off); tw: the
    // widened bound (B0)
    void cull_targets(size_t i, const OpenUnion &u, const std::string &P) {
        const std::string D = std::to_string(u.depth);
        o << "    const bool pb" << D << " = fmaxf(fmaxf(fabsf(x" << D << "), fabsf(y" << D << ")), fabsf(z" << D
          << ")) < 0x1p40f;\n";
        if (u.use_bnd)
            o << "    const float tg" << D << " = cull_target(h" << P << ".d, bnd) * " << ref(i) << ".pad[0];\n";
        else if (!v.bound_rule)
            // out-of-range point: a NaN target, which every test fails
            // (the same decisions as `pb & test`); cT: the target's
            // margin term for the union's unscaled shapes
            o << "    const float tg" << D << " = pb" << D << " ? h" << P << ".d * " << ref(i)
              << ".pad[0] : __builtin_nanf(\"\");\n"
              << "    const float cT" << D << " = " << margin("tg" + D) << ";\n";
        else
            o << "    const float tg" << D << " = h" << P << ".d * " << ref(i) << ".pad[0];\n";
        if (v.records_live && info[i].live_mask)
            o << "    const float tw" << D << " = bndw * " << ref(i) << ".pad[0];\n";
    }

    void shape(size_t i) {
        OpenUnion &u = open.back();
        u.fresh = false;
        // culled shapes: those of a union that combines into its parent by
        // union (assign/union shapes only), against the parent's running
        // distance.  (Also testing against the union's own running
        // distance measured slower: the test then waits for the previous
        // shape's combine.)
        if (u.cull_on && u.masked) shape_by_live_bit(i, u);
        else if (u.cull_on) shape_culled(i, u);
        else shape_plain(i, u);
    }

    // B1: the live mask decides.  B0 sets a live bit only
    // inside the shape's check[] test, so a live lane needs no check test of
    // its own; the check[] bit matters only for a dropped first (assign) shape
    // and for the counters.
    void shape_by_live_bit(size_t i, const OpenUnion &u) {
        const PtNode &n = nodes[i];
        const std::string D = std::to_string(u.depth);
        o << "    {  // shape " << i << "\n"
          << "      if ((live >> " << info[i].live_bit << ") & 1ull) {\n"
          << "        if constexpr (ST) " << count_shape(n) << ";\n"
          << "        count_eval(st);\n"
          << "        float x = x" << D << ", y = y" << D << ", z = z" << D << ";\n"
          << "        xform_f<" << n.flags << "u>(" << ref(i) << ", x, y, z);\n"
          << "        float d = " << sdf_call(i) << ";\n";
        shape_tail("        ", i, D);
        o << "      } else {\n"  // a lane without the live bit
          << "        if constexpr (ST) {\n"
          << "          if (" << check_test(n) << ") {\n"
          << "            " << count_shape(n) << ";\n"
          << "            st.add(PT_ST_CULLED);\n"
          << "          }\n"
          << "        }\n";
        if (n.combine == PT_COMBINE_ASSIGN) o << "        if (" << check_test(n) << ") " << drop_assign(D, n) << "\n";
        o << "      }\n"
          << "    }\n";
    }

    // Inside the check[] branch: skip when |t|, t = p/s - pos/s, proves d > tg,
    // the parent's running distance (or the map() bound) in this union's frame
    // (DESIGN.md 3.12).  JitMapB*: a cube also when max(q) > tg after its
    // rotation (sdCube >= max(q) in f32); the cubes of a fresh
    // union (target from the bound only) take just that test, their radius
    // bound being too loose for slabs such as C3's walls.  B0 also records the
    // shape in `live` unless the same tests against tw (the bound widened by
    // the taps' spread) fire.
    void shape_culled(size_t i, const OpenUnion &u) {
        const PtNode &n = nodes[i];
        const std::string D = std::to_string(u.depth);
        const bool cube_test = v.bound_rule && n.shape == PT_NODE_CUBE;
        const bool radius = !(cube_test && u.parent_fresh);
        const bool record = v.records_live && info[u.begin].live_mask != 0;
        const uint32_t pre = n.flags & (PT_NF_SCALE | PT_NF_POS), rot = n.flags & ~pre;
        shape_open(i, D, pre);
        o << "      const float ca = tg" << D << times_inv(i) << ";\n";
        if (record)
            o << "      const float cw = tw" << D << times_inv(i) << ";\n"
              << "      bool keep = true;\n";
        o << "      " << count_shape(n) << ";\n";
        if (radius) {
            radius_test(i, D, record);
            o << "      if (!cut) {\n";
        } else {
            o << "      {\n";
        }
        if (!cube_test) o << "        count_eval(st);\n";
        o << "        xform_f<" << rot << "u>(" << ref(i) << ", x, y, z);\n";
        if (cube_test) {
            cube_test_and_sdf(i, D, record);
        } else {
            o << "        float d = " << sdf_call(i) << ";\n";
            shape_tail("        ", i, D);
        }
        o << "      }\n";
        if (record) o << "      if (keep) live |= 1ull << " << info[i].live_bit << ";\n";
        o << "    }\n";
    }

    // cut: |t|^2 (1 - 2^-10) > (target + margin + R')^2.  The trace map's
    // target is NaN for an out-of-range point and its unscaled shapes take the
    // union's hoisted cT = fma(|tg|, 2^-12, tg); the taps' maps join pb by `&`.
    void radius_test(size_t i, const std::string &D, bool record) {
        const PtNode &n = nodes[i];
        const bool hoisted = !v.bound_rule && !(n.flags & PT_NF_SCALE);
        o << "      const float cK = " << (hoisted ? "cT" + D : margin("ca")) << " + " << ref(i) << ".pad[0];\n"
          << "      const float cl = __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x));\n";
        if (!v.bound_rule) o << "      const bool cut = cl * 0x1.ff8p-1f > cK * cK;\n";
        else o << "      const bool cut = pb" << D << " & (cl * 0x1.ff8p-1f > cK * cK);\n";
        if (record)
            o << "      const float cKw = " << margin("cw") << " + " << ref(i) << ".pad[0];\n"
              << "      keep = !(pb" << D << " & (cl * 0x1.ff8p-1f > cKw * cKw));\n";
        o << "      if (cut) st.add(PT_ST_CULLED);\n";
        if (n.combine == PT_COMBINE_ASSIGN) o << "      if (cut) " << drop_assign(D, n) << "\n";
    }

    void cube_test_and_sdf(size_t i, const std::string &D, bool record) {
        const PtNode &n = nodes[i];
        cube_q("        ", i);
        o << "        const float cq = " << margin("ca") << ";\n"
          << "        const bool cut_q = qm > cq && qm > 0x1p-60f;  // NaN target: no cut\n";
        if (record)
            o << "        const float cqw = " << margin("cw") << ";\n"
              << "        keep = keep && !(qm > cqw && qm > 0x1p-60f);\n";
        o << "        if (cut_q) st.add(PT_ST_CULLED);\n";
        if (n.combine == PT_COMBINE_ASSIGN) o << "        if (cut_q) " << drop_assign(D, n) << "\n";
        o << "        if (!cut_q) {\n"
          << "          count_eval(st);\n"
          << "          float d = " << cube_from_q(i) << ";\n";
        shape_tail("          ", i, D);
        o << "        }\n";
    }

    void shape_plain(size_t i, const OpenUnion &u) {
        const PtNode &n = nodes[i];
        const std::string D = std::to_string(u.depth);
        shape_open(i, D, n.flags);
        if (!v.bound_rule && n.shape == PT_NODE_CUBE && n.combine == PT_COMBINE_UNION && !(n.flags & PT_NF_SCALE)) {
            // the trace map, a cube joining its union by min: sdCube >= max(q)
            // in f32 (3.13), so max(q) > the union's running distance proves
            // the min unchanged -- the lane skips the rest of the SDF
            cube_q("      ", i);
            o << "      " << count_shape(n) << ";\n"
              // (qm > 2^-60: below it RN(qm^2) may underflow and
              // sdCube >= max(q) fails, as for cut_q)
              << "      const bool cut_r = (qm > h" << D << ".d) & (qm > 0x1p-60f);\n"
              << "      if (cut_r) st.add(PT_ST_CULLED);\n"
              << "      if (!cut_r) {\n"
              << "        count_eval(st);\n"
              << "        const float d = " << cube_from_q(i) << ";\n";
            shape_tail("        ", i, D);
            o << "      }\n"
              << "    }\n";
            return;
        }
        o << "      float d = " << sdf_call(i) << ";\n";
        shape_tail("      ", i, D);
        o << "      " << count_shape(n) << ";\n"
          << "      count_eval(st);\n"
          << "    }\n";
    }

    void union_end(size_t i) {
        const OpenUnion u = open.back();
        open.pop_back();
        open.back().fresh = false;
        const std::string D = std::to_string(u.depth), P = std::to_string(u.depth - 1);
        if (u.masked) {
            // a skipped union still counts its shapes (algorithmic work =
            // the oracle's); its first shape, when check[] admits it, is
            // dropped as +inf (it would have overwritten MAXHIT)
            o << "    } else {  // live\n";
            for (size_t j = u.begin + 1; j < i; ++j)
                if (nodes[j].combine == PT_COMBINE_ASSIGN)
                    o << "      " << check_guard(nodes[j], v.wave_guards) << drop_assign(D, nodes[j]) << "\n";
            o << "      if constexpr (ST) {\n";
            for (size_t j = u.begin + 1; j < i; ++j)
                o << "        " << check_guard(nodes[j], v.wave_guards) << count_culled(nodes[j]) << "\n";
            o << "      }\n"
              << "    }\n";
        }
        o << "    {\n"
          << "      float d = h" << D << ".d;\n";
        divide("      ", i);
        combine_parent("      ", nodes[i], P, "Hit{d, h" + D + ".m}");
        o << "    }\n";
        if (u.skipped) o << "    }  // (the wave needs a shape of it)\n";
        o << "    }  // end union\n";
    }
};

// ---- the rest of the scene's source -------------------------------------------------

// A/B experiments on the embedded headers (the one experiment hook; the
// shipped kernels define nothing): PT_JIT_DEFS="A,B=1" -> #define A /
// #define B 1.  The defines are part of the source, so of the cache key.
void emit_experiment_defs(std::ostringstream &o) {
    const char *defs = std::getenv("PT_JIT_DEFS");
    if (!defs) return;
    std::string tok;
    std::istringstream is(defs);
    while (std::getline(is, tok, ',')) {
        if (tok.empty()) continue;
        const size_t eq = tok.find('=');
        o << "#define " << (eq == std::string::npos ? tok : tok.substr(0, eq) + " " + tok.substr(eq + 1)) << "\n";
    }
}

const char *kJitTaps =
    "struct JitTaps {  // the shade pass's six taps: B0 for the first, B1 for the rest\n"
    "  static __device__ __forceinline__ uint64_t alive(uint64_t) { return ~0ull; }\n"
    "  template <bool ST>\n"
    "  static __device__ __forceinline__ Hit first(const PtLaunch &L, float qx, float qy, float qz, const Check &ck,\n"
    "                                              float bnd, float bndw, uint64_t &live, Stats<ST> &st) {\n"
    "    return JitMapB0::eval<ST>(L, qx, qy, qz, ck, bnd, bndw, live, st);\n"
    "  }\n"
    "  template <bool ST>\n"
    "  static __device__ __forceinline__ Hit rest(const PtLaunch &L, float qx, float qy, float qz, const Check &ck,\n"
    "                                             float bnd, float bndw, uint64_t &live, Stats<ST> &st) {\n"
    "    return JitMapB1::eval<ST>(L, qx, qy, qz, ck, bnd, bndw, live, st);\n"
    "  }\n"
    "};\n";

// bounds() of the shade pass, straight-line: one slab test per box with
// its check[] bit as a constant (and, baked, the box as literals), the
// same f32 steps as pt_binned.h bounds_mask (test_compute.glsl:101,
// sdf_editor.rs:224-238), so the same bits.
// Slab values from the reciprocal products, decided by the ulp margin
// (+1.2 % over the float margin of 3.14); a wave with an
// undecided lane redoes every box with the exact Markstein values (3.10)
// for those lanes.  Each box's bit is a select OR-ed into its word
// (v_cndmask + v_or3 for two boxes).
// mask_skip: the same with the fast path's box k left out where bit k
// of `skip` is set (the first pass's camera rays: primary_box_skip,
// DESIGN.md 3.20); mask() passes no skip, which folds the guards away
void emit_map_bounds(std::ostringstream &o, const std::vector<PtAabb> &boxes, bool fast_bounds, bool bake) {
    o << "template <> struct MapBounds<JitTaps> {\n"
         "  template <bool ST>\n"
         "  static __device__ __forceinline__ uint4 mask(const PtLaunch &L, const pt_f3 &ro, const pt_f3 &rd,\n"
         "                                              Stats<ST> &st) {\n"
         "    return mask_skip<ST>(L, ro, rd, 0ull, st);\n"
         "  }\n"
         "  template <bool ST>\n"
         "  static __device__ __forceinline__ uint4 mask_skip(const PtLaunch &L, const pt_f3 &ro, const pt_f3 &rd,\n"
         "                                                   uint64_t skip, Stats<ST> &st) {\n"
         "    (void)skip;\n"
         "    uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;\n"
         "    const caabb_ptr boxes = (caabb_ptr)L.aabbs;\n"
         "    (void)boxes;\n";
    if (bake)
        for (size_t k = 0; k < boxes.size(); ++k) {
            const PtAabb &b = boxes[k];
            o << "    constexpr PtAabb A" << k << "{{" << hexf(b.bmin[0]) << ", " << hexf(b.bmin[1]) << ", "
              << hexf(b.bmin[2]) << "}, {" << hexf(b.bmax[0]) << ", " << hexf(b.bmax[1]) << ", " << hexf(b.bmax[2])
              << "}, " << b.back << ", 0};\n";
        }
    auto box = [&](size_t k) { return bake ? "A" + std::to_string(k) : "boxes[" + std::to_string(k) + "]"; };
    // box k's check[] bit: word index and the bit within it
    auto word = [&](size_t k) { return uint32_t(boxes[k].back) >> 5; };
    auto bit = [&](size_t k) { return hex_lit(1u << (uint32_t(boxes[k].back) & 31u), "u"); };
    o << "    const bool fast = " << (bake ? (fast_bounds ? "true" : "false") : "L.fast_bounds != 0")
      // (& not &&: six compares and no branch per guard)
      << " && (pt_div_coord_ok(ro.x) & pt_div_coord_ok(ro.y) &\n"
         "                      pt_div_coord_ok(ro.z) & pt_div_dir_ok(rd.x) & pt_div_dir_ok(rd.y) & pt_div_dir_ok(rd.z));\n"
         "    if (fast) {\n"
         "      if constexpr (ST)\n"
         "        if (first_active_lane()) st.add(PT_ST_BOUNDS_WAVES);\n"
         "      const float yx = 1.0f / rd.x, yy = 1.0f / rd.y, yz = 1.0f / rd.z;\n"
         "      uint32_t gapu = 0xffffffffu;\n";
    for (size_t k = 0; k < boxes.size(); ++k) {
        // (boxes 64 and up take no skip bit: primary_box_skip covers at most 64)
        if (k < 64) o << "      if (!((skip >> " << k << ") & 1ull))";
        else o << "     ";
        o << " w" << word(k) << " |= ray_box_ulp(" << box(k) << ", ro.x, ro.y, ro.z, yx, yy, yz, gapu) ? " << bit(k)
          << " : 0u;\n";
    }
    // (the origin passes through an empty asm so the exact path's slab
    // differences are not shared with the approximate ones, which would
    // keep all of them live across both; the exact masks go to v0..v3 and
    // replace w only in the undecided lanes)
    o << "      if (__builtin_expect(__ballot(!(gapu > PT_ULP_MARGIN)) != 0ull, 0)) {\n"
         "        if constexpr (ST)\n"
         "          if (first_active_lane()) st.add(PT_ST_BOUNDS_EXACT);\n"
         "        uint32_t v0 = 0u, v1 = 0u, v2 = 0u, v3 = 0u;\n"
         "        float ex = ro.x, ey = ro.y, ez = ro.z;\n"
         "        __asm__ volatile(\"\" : \"+v\"(ex), \"+v\"(ey), \"+v\"(ez));\n";
    for (size_t k = 0; k < boxes.size(); ++k)
        o << "      if (ray_box_rcp(" << box(k) << ", ex, ey, ez, rd.x, rd.y, rd.z, yx, yy, yz)) v" << word(k)
          << " |= " << bit(k) << ";\n";
    o << "        if (!(gapu > PT_ULP_MARGIN)) {\n"
         "          w0 = v0;\n"
         "          w1 = v1;\n"
         "          w2 = v2;\n"
         "          w3 = v3;\n"
         "        }\n"
         "      }\n"
         "    } else {\n";
    for (size_t k = 0; k < boxes.size(); ++k)
        o << "      if (ray_box(" << box(k) << ", ro.x, ro.y, ro.z, rd.x, rd.y, rd.z)) w" << word(k) << " |= " << bit(k)
          << ";\n";
    o << "    }\n"
         "    st.add(PT_ST_SEGMENTS);\n"
         "    st.add(PT_ST_AABB, " << boxes.size() << "u);\n"
         "    return make_uint4(w0, w1, w2, w3);\n"
         "  }\n"
         "};\n"
         // the trace pass's own primary rays (PtPass gen_trace) take the same bounds()
         "template <> struct MapBounds<JitMap> : MapBounds<JitTaps> {};\n";
}

void emit_traits(std::ostringstream &o, const std::vector<PtNode> &nodes, const std::vector<PtAabb> &boxes) {
    // check[] width: narrow scenes' kernels drop the high mask words
    bool wide = false;
    for (const PtNode &n : nodes) wide = wide || n.check >= 64;
    for (const PtAabb &b : boxes) wide = wide || b.back >= 64;
    for (const char *m : {"JitMap", "JitTaps"})
        o << "template <> struct MapWide<" << m << "> {\n  static constexpr int v = " << (wide ? 1 : 0) << ";\n};\n";
    // The material table (up to 64 entries = 3 KB) is staged in LDS by the
    // shade pass (+0.4 %)
    int n_mat = 1;  // (entry 0: the default material)
    for (const PtNode &n : nodes)
        if (n.op == PT_OP_SHAPE) n_mat = std::max(n_mat, int(n.mat) + 1);
    if (n_mat <= 64) o << "template <> struct MapMats<JitTaps> {\n  static constexpr int n = " << n_mat << ";\n};\n";
}

// waves per SIMD of the binned kernels (the compile's -D fallback overrides
// the default per kernel: PT_TW_N the march-only pass, PT_TG_N the first
// pass, PT_TT_N the pass with the taps in it, PT_SW_N the shade pass; it
// lowers only the ones that spilled)
void emit_waves_macros(std::ostringstream &o) {
    o << "#define PT_WAVES\n";
    o << "#ifndef PT_TW_N\n#define PT_TW_N " << kJitWaves << "\n#endif\n"
      << "#ifndef PT_TG_N\n#define PT_TG_N PT_TW_N\n#endif\n"
      << "#ifndef PT_TT_N\n#define PT_TT_N PT_TW_N\n#endif\n"
      << "#define PT_TRACE_WAVES __attribute__((amdgpu_waves_per_eu(PT_TW_N)))\n"
      << "#define PT_TRACEG_WAVES __attribute__((amdgpu_waves_per_eu(PT_TG_N)))\n"
      << "#define PT_TRACET_WAVES __attribute__((amdgpu_waves_per_eu(PT_TT_N)))\n"
      << "#ifndef PT_SW_N\n#define PT_SW_N " << kJitWaves << "\n#endif\n"
      << "#define PT_SHADE_WAVES __attribute__((amdgpu_waves_per_eu(PT_SW_N)))\n"
      // the posed-camera builds of the first pass and of shade pass 0 (pt_path.h
      // PT_CAMK_POSED) carry the ray's origin in registers where the fixed
      // camera's is a constant: 7 waves (72 VGPRs) from the start, so that they
      // never cost a scene its second compile
      << "#define PT_POSED_WAVES __attribute__((amdgpu_waves_per_eu(" << (kJitWaves - 1) << ")))\n";
}

void emit_kernels(std::ostringstream &o) {
    for (const PtJitKernel &k : kJitKernels) {
        o << "extern \"C\" __global__ __launch_bounds__(" << k.bounds << ") ";
        if (k.waves) o << k.waves << " ";
        o << "void " << k.name << "(" << k.param << ") {\n  " << k.body << ";\n}\n";
    }
}

}  // namespace

// the scene's source up to and including the wave macros: what the scene kernels
// (pt_jit_source) and the probe kernels (pt_probe_source) are both built on
static void emit_scene(std::ostringstream &o, const std::vector<PtNode> &nodes, const std::vector<PtAabb> &boxes,
                       bool fast_bounds, bool bake) {
    const std::vector<NodeInfo> info = analyse(nodes);
    o << "// generated by pt_jit.cpp from the scene op list\n";
    emit_experiment_defs(o);
    o << "#include \"pt_wave.h\"\n"
         "#include \"pt_binned.h\"\n"
         "namespace pt {\n";
    for (const MapVariant &v : kMapVariants) MapEmitter(o, nodes, info, bake, v).emit();
    o << kJitTaps;
    emit_map_bounds(o, boxes, fast_bounds, bake);
    emit_traits(o, nodes, boxes);
    o << "}  // namespace pt\n";
    emit_waves_macros(o);
}

std::string pt_jit_source(const std::vector<PtNode> &nodes, const std::vector<PtAabb> &boxes, bool fast_bounds,
                          bool bake) {
    std::ostringstream o;
    emit_scene(o, nodes, boxes, fast_bounds, bake);
    emit_kernels(o);
    return o.str();
}

// A probe module's source: the scene's own map() variants and
// bounds(), text for text, with probe kernels of pt_map_probe.h in place of
// the scene kernels -- the one kernel (fn, stats) a probe call needs, so a call
// compiles no more than it runs, or all of them (fn < 0).
std::string pt_probe_source(const std::vector<PtNode> &nodes, const std::vector<PtAabb> &boxes, bool fast_bounds,
                            bool bake, int fn, bool stats) {
    std::ostringstream o;
    emit_scene(o, nodes, boxes, fast_bounds, bake);
    o << "#include \"pt_map_probe.h\"\n";
    for (const PtProbeKernel &k : kProbeKernels)
        for (int st = 0; st < 2; ++st)
            if (fn < 0 || (k.fn == fn && (st != 0) == stats))
                o << "extern \"C\" __global__ __launch_bounds__(64) void " << k.name << (st ? "_stats" : "")
                  << "(PtProbe P) {\n  pt::" << k.body << ", " << (st ? "true" : "false") << ">(P);\n}\n";
    return o.str();
}

int pt_derive_source(const pt_op *ops, uint32_t n_ops, const pt_aabb *aabbs, uint32_t n_aabb, const float *data,
                     uint32_t n_data, bool bake, PtDerived &t, std::string &src, std::string &err) {
    const std::vector<pt_op> o(ops, ops + n_ops);
    const std::vector<pt_aabb> a(aabbs, aabbs + n_aabb);
    const int rc = pt_derive(o, a, data, n_data, t.nodes, t.boxes, t.mats, err);
    if (rc == PT_OK) src = pt_jit_source(t.nodes, t.boxes, pt_fast_bounds(t.boxes), bake);
    return rc;
}

// The generated scene-kernel source for (program, data) without compiling
// it -- the counterpart of the reference's dump of its spliced shader to
// shader_out/test_compute.glsl (glsl_preprocessor.rs:5-15).  Host only.
// Two-call pattern: *len = bytes including the terminating NUL; `out` may
// be NULL; a `cap` below *len returns PT_ERR_SIZE.
extern "C" int pt_scene_kernel_source(const pt_op *ops, uint32_t n_ops, const pt_aabb *aabbs, uint32_t n_aabb,
                                      const float *data, uint32_t n_data, int baked, char *out, size_t cap,
                                      size_t *len) {
    if ((!ops && n_ops) || (!aabbs && n_aabb) || (!data && n_data) || !len) return PT_ERR_INVALID;
    PtDerived t;
    std::string src, err;
    const int rc = pt_derive_source(ops, n_ops, aabbs, n_aabb, data, n_data, baked != 0, t, src, err);
    if (rc != PT_OK) return rc;
    *len = src.size() + 1;
    if (!out) return PT_OK;
    if (cap < *len) return PT_ERR_SIZE;
    std::memcpy(out, src.c_str(), src.size() + 1);
    return PT_OK;
}

// The probe module's source for (program, data), as pt_scene_kernel_source
// returns the scene kernels': the same text up to the kernel list.
extern "C" int pt_probe_kernel_source(const pt_op *ops, uint32_t n_ops, const pt_aabb *aabbs, uint32_t n_aabb,
                                      const float *data, uint32_t n_data, int baked, char *out, size_t cap,
                                      size_t *len) {
    if ((!ops && n_ops) || (!aabbs && n_aabb) || (!data && n_data) || !len) return PT_ERR_INVALID;
    PtDerived t;
    std::string src, err;
    const int rc = pt_derive_source(ops, n_ops, aabbs, n_aabb, data, n_data, baked != 0, t, src, err);
    if (rc != PT_OK) return rc;
    src = pt_probe_source(t.nodes, t.boxes, pt_fast_bounds(t.boxes), baked != 0);
    *len = src.size() + 1;
    if (!out) return PT_OK;
    if (cap < *len) return PT_ERR_SIZE;
    std::memcpy(out, src.c_str(), src.size() + 1);
    return PT_OK;
}
