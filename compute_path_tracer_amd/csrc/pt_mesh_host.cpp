// pt_mesh_host.cpp -- the mesh export entry points of include/pt_abi.h:
// pt_sample_field, pt_mesh_extract, pt_mesh_read.  Kernels in
// pt_mesh.hip; every launch on the context's stream.  Nothing here touches
// the accumulation image, the guides, the camera, the sky or an option.
#include <cmath>
#include <cstring>

#include "pt_ctx.h"
#include "pt_mesh.h"

static_assert(sizeof(pt_mesh_desc) == 36, "pt_mesh_desc layout");
static_assert(sizeof(pt_mesh_info) == 48, "pt_mesh_info layout");
static_assert(PT_MESH_BRICK == 8, "a brick's 512 cells are one workgroup's threads, 64 per mask word");

static PtMeshScene mesh_scene(const pt_ctx *c) {
    return PtMeshScene{c->prog.nodes.as<PtNode>(), int32_t(c->prog.ops.size()), c->prog.bound_k};
}

extern "C" {

int pt_sample_field(pt_ctx *c, const float *xyz, uint32_t n, float *d, int32_t *shape) {
    if (!c) return PT_ERR_INVALID;
    if (n && !xyz) return fail(c, PT_ERR_INVALID, "null points");
    if (!c->prog.have_program || !c->prog.have_data) return fail(c, PT_ERR_STATE, "no program/data uploaded");
    if (!n) return PT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    pt_ctx::Mesher &m = c->mesh;
    int rc;
    if ((rc = ensure(c, m.sample_xyz, size_t(n) * 12)) != PT_OK) return rc;
    if (d && (rc = ensure(c, m.sample_d, size_t(n) * 4)) != PT_OK) return rc;
    if (shape && (rc = ensure(c, m.sample_shape, size_t(n) * 4)) != PT_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(m.sample_xyz.p, xyz, size_t(n) * 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, m.sample_time.begin(c->stream));
    pt_launch_sample(mesh_scene(c), m.sample_xyz.as<float>(), n, d ? m.sample_d.as<float>() : nullptr,
                     shape ? m.sample_shape.as<int32_t>() : nullptr, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, m.sample_time.end(c->stream));
    if (d) HIPCHK(c, hipMemcpyAsync(d, m.sample_d.p, size_t(n) * 4, hipMemcpyDeviceToHost, c->stream));
    if (shape) HIPCHK(c, hipMemcpyAsync(shape, m.sample_shape.p, size_t(n) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_mesh_extract(pt_ctx *c, const pt_mesh_desc *g, pt_mesh_info *info) {
    if (!c) return PT_ERR_INVALID;
    if (!g || !info) return fail(c, PT_ERR_INVALID, "null mesh description / info");
    for (float v : {g->origin[0], g->origin[1], g->origin[2], g->cell, g->iso})
        if (!std::isfinite(v)) return fail(c, PT_ERR_INVALID, "mesh origin, cell and iso must be finite");
    if (!(g->cell > 0.0f)) return fail(c, PT_ERR_INVALID, "mesh cell must be > 0");
    for (uint32_t n : g->cells)
        if (n < 1 || n > PT_MESH_MAX_CELLS) return fail(c, PT_ERR_INVALID, "mesh cells must be in [1, 1024] per axis");
    if (g->project > PT_MESH_MAX_PROJECT) return fail(c, PT_ERR_INVALID, "mesh project must be in [0, 8]");
    if (!c->prog.have_program || !c->prog.have_data) return fail(c, PT_ERR_STATE, "no program/data uploaded");
    HIPCHK(c, hipSetDevice(c->device));

    PtMeshGrid G;
    std::memset(&G, 0, sizeof G);
    G.n_bricks = 1;
    for (int a = 0; a < 3; ++a) {
        G.origin[a] = g->origin[a];
        G.n[a] = g->cells[a];
        G.nb[a] = (g->cells[a] + PT_MESH_BRICK - 1) / PT_MESH_BRICK;
        G.n_bricks *= G.nb[a];  // (at most 128^3)
    }
    G.cell = g->cell;
    G.iso = g->iso;
    G.project = g->project;
    const PtMeshScene S = mesh_scene(c);
    pt_ctx::Mesher &m = c->mesh;
    using M = pt_ctx::Mesher;
    int rc;
    // per brick: 12 B
    for (DevBuf *b : {&m.flag, &m.slot, &m.list})
        if ((rc = ensure(c, *b, size_t(G.n_bricks) * 4)) != PT_OK) return rc;
    if ((rc = ensure(c, m.ctr, sizeof(unsigned long long) * PT_MC_COUNT)) != PT_OK) return rc;
    PtMeshBufs B;
    std::memset(&B, 0, sizeof B);
    B.flag = m.flag.as<uint32_t>();
    B.slot = m.slot.as<int32_t>();
    B.list = m.list.as<uint32_t>();
    B.ctr = m.ctr.as<unsigned long long>();
    unsigned long long ctr[PT_MC_COUNT];

    // stage 1: the skip test and the brick -> slot scan
    HIPCHK(c, hipMemsetAsync(m.ctr.p, 0, sizeof ctr, c->stream));
    HIPCHK(c, m.stage_time[M::kSkip].begin(c->stream));
    pt_launch_mesh_skip(S, G, B, m.skip != 0, c->stream);
    pt_launch_mesh_slots(G, B, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, m.stage_time[M::kSkip].end(c->stream));
    HIPCHK(c, hipMemcpyAsync(ctr, m.ctr.p, sizeof ctr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t n_eval = uint32_t(ctr[PT_MC_SLOTS]);
    if (n_eval > G.n_bricks) return fail(c, PT_ERR_HIP, "mesh slot scan out of range");

    // per evaluated brick: 2916 B of lattice, 256 B of masks, 16 B of counts and bases
    const size_t ne = n_eval;
    if ((rc = ensure(c, m.lattice, ne * PT_MESH_LAT3 * 4)) != PT_OK) return rc;
    if ((rc = ensure(c, m.vmask, ne * PT_MESH_WORDS * 8)) != PT_OK) return rc;
    if ((rc = ensure(c, m.qmask, ne * 3 * PT_MESH_WORDS * 8)) != PT_OK) return rc;
    for (DevBuf *b : {&m.nv, &m.nt, &m.vbase, &m.tbase})
        if ((rc = ensure(c, *b, ne * 4)) != PT_OK) return rc;
    B.lattice = m.lattice.as<float>();
    B.vmask = m.vmask.as<uint64_t>();
    B.qmask = m.qmask.as<uint64_t>();
    B.nv = m.nv.as<uint32_t>();
    B.nt = m.nt.as<uint32_t>();
    B.vbase = m.vbase.as<uint32_t>();
    B.tbase = m.tbase.as<uint32_t>();

    // stages 2 and 3: classify, count, scan
    HIPCHK(c, m.stage_time[M::kClassify].begin(c->stream));
    pt_launch_mesh_classify(S, G, B, n_eval, c->stream);
    pt_launch_mesh_count(G, B, n_eval, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, m.stage_time[M::kClassify].end(c->stream));
    HIPCHK(c, m.stage_time[M::kScan].begin(c->stream));
    pt_launch_mesh_scan(B, n_eval, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, m.stage_time[M::kScan].end(c->stream));
    HIPCHK(c, hipMemcpyAsync(ctr, m.ctr.p, sizeof ctr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned long long nv = ctr[PT_MC_VERTS], nt = ctr[PT_MC_TRIS];
    if (nv >= (1ull << 31) || nt >= (1ull << 31))
        return fail(c, PT_ERR_UNSUPPORTED, "mesh would reach 2^31 vertices or triangles");

    // stage 4: emit into the snapshot's buffers (from here on the previous mesh is gone)
    m.have = false;
    if ((rc = ensure(c, m.pos, size_t(nv) * 12)) != PT_OK) return rc;
    if ((rc = ensure(c, m.nrm, size_t(nv) * 12)) != PT_OK) return rc;
    if ((rc = ensure(c, m.shp, size_t(nv) * 4)) != PT_OK) return rc;
    if ((rc = ensure(c, m.tri, size_t(nt) * 12)) != PT_OK) return rc;
    if ((rc = ensure(c, m.vcell, size_t(nv) * 4)) != PT_OK) return rc;
    B.pos = m.pos.as<float>();
    B.nrm = m.nrm.as<float>();
    B.shp = m.shp.as<int32_t>();
    B.tri = m.tri.as<uint32_t>();
    B.vcell = m.vcell.as<uint32_t>();
    HIPCHK(c, m.stage_time[M::kEmit].begin(c->stream));
    pt_launch_mesh_emit(S, G, B, n_eval, uint32_t(nv), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, m.stage_time[M::kEmit].end(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    m.n_vertices = size_t(nv);
    m.n_triangles = size_t(nt);
    m.have = true;

    pt_mesh_info out;
    std::memset(&out, 0, sizeof out);
    out.n_vertices = uint32_t(nv);
    out.n_triangles = uint32_t(nt);
    out.clipped_edges = uint32_t(ctr[PT_MC_CLIPPED]);
    out.void_cells = uint32_t(ctr[PT_MC_VOID]);
    out.dropped_quads = uint32_t(ctr[PT_MC_DROPPED]);
    out.bricks = G.n_bricks;
    out.bricks_evaluated = n_eval;
    out.corner_evals = ctr[PT_MC_EVALS];
    out.device_bytes = m.bytes();
    *info = out;
    return PT_OK;
}

int pt_mesh_read(pt_ctx *c, float *positions, float *normals, int32_t *shapes, uint32_t *triangles, size_t vertex_cap,
                 size_t triangle_cap) {
    if (!c) return PT_ERR_INVALID;
    const pt_ctx::Mesher &m = c->mesh;
    if (!m.have) return fail(c, PT_ERR_STATE, "no mesh: call pt_mesh_extract");
    if ((positions || normals || shapes) && vertex_cap < m.n_vertices) return fail(c, PT_ERR_SIZE, "vertex buffers too small");
    if (triangles && triangle_cap < m.n_triangles) return fail(c, PT_ERR_SIZE, "triangle buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nv = m.n_vertices, nt = m.n_triangles;
    if (positions && nv) HIPCHK(c, hipMemcpyAsync(positions, m.pos.p, nv * 12, hipMemcpyDeviceToHost, c->stream));
    if (normals && nv) HIPCHK(c, hipMemcpyAsync(normals, m.nrm.p, nv * 12, hipMemcpyDeviceToHost, c->stream));
    if (shapes && nv) HIPCHK(c, hipMemcpyAsync(shapes, m.shp.p, nv * 4, hipMemcpyDeviceToHost, c->stream));
    if (triangles && nt) HIPCHK(c, hipMemcpyAsync(triangles, m.tri.p, nt * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

}  // extern "C"
