// pt_mesh.hip -- mesh export for CDNA4 (gfx950): pt_sample_field's field
// sampling and the surface-nets extractor of pt_mesh_extract, beside the render
// kernels (DESIGN.md 3.27 is the contract: every f32 step and every order).
//
//   mesh_sample_kernel    one thread per caller point: map() with every check[] true
//   mesh_skip_kernel      one thread per 8x8x8-cell brick: map() at its centre; a brick whose
//                         centre value exceeds its half-diagonal (plus the f32 margin) holds no surface
//   mesh_scan_kernel      one workgroup: exclusive prefix sums (brick -> slot; the bricks'
//                         vertex and triangle bases), so every order comes from a scan, none from atomics
//   mesh_classify_kernel  one workgroup per surviving brick: its 9^3 corner lattice into LDS (and to
//                         memory for the emit stage), the cells with a vertex and the sign-changing
//                         edges as wave ballots
//   mesh_count_kernel     the same grid: which of those edges emit a quad (all four cells around
//                         them have a vertex), read from the neighbours' masks
//   mesh_emit_kernel      the same grid: triangles, and each vertex's cell; a neighbour's vertex index =
//                         its brick's base + popcount of the mask bits below it
//   mesh_vertex_kernel    one thread per vertex, in full waves: crossing mean, projection, normal, shape
// No workgroup waits on another: stage boundaries are launch boundaries.  map()
// is the op-list interpreter (InterpMap) in every kernel.
#include "pt_path.h"
#include "pt_mesh.h"

namespace pt {

// map() at one point, every check[] entry true.  A point with a non-finite
// coordinate is (NaN, NaN, NaN): the reference multiplies by three full rotation
// matrices per union (shapes.glsl:34-68), zeros included, and 0 * inf = 0 * NaN
// = NaN; the interpreter skips the zero terms and would keep the other
// coordinates (pt_derive.cpp does the same for a non-finite transform).
__device__ __noinline__ Hit mesh_map(const PtNode *nodes, int32_t n_nodes, float x, float y, float z) {
    if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))) x = y = z = __builtin_nanf("");
    PtLaunch L;
    L.nodes = nodes;
    L.n_nodes = n_nodes;
    const Check all{~0ull, ~0ull};
    Stats<false> st;
    return map_plain<InterpMap, false>(L, x, y, z, all, st);
}

// calc_normal (pt_path.h; funcs.glsl:21-35) over mesh_map, normalised
__device__ __forceinline__ float mesh_dist(float x, float y, float z, const PtNode *nodes, int32_t n_nodes) {
    return mesh_map(nodes, n_nodes, x, y, z).d;
}
__device__ pt_f3 mesh_normal(const PtNode *nodes, int32_t n_nodes, pt_f3 p) {
    return pt_normalize(calc_normal<mesh_dist>(p, nodes, n_nodes));
}

__global__ __launch_bounds__(256) void mesh_sample_kernel(PtMeshScene S, const float *__restrict__ xyz, uint32_t n,
                                                          float *__restrict__ d, int32_t *__restrict__ shape) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const Hit h = mesh_map(S.nodes, S.n_nodes, xyz[3 * size_t(i)], xyz[3 * size_t(i) + 1], xyz[3 * size_t(i) + 2]);
    if (d) d[i] = h.d;
    if (shape) shape[i] = h.m - 1;
}

// corner index -> coordinate: one multiply, one add (the build contracts nothing)
__device__ __forceinline__ float corner_pos(const PtMeshGrid &G, int a, uint32_t idx) {
    return G.origin[a] + float(idx) * G.cell;
}

__device__ __forceinline__ void brick_coords(const PtMeshGrid &G, uint32_t b, uint32_t bc[3]) {
    bc[0] = b % G.nb[0];
    bc[1] = (b / G.nb[0]) % G.nb[1];
    bc[2] = b / (G.nb[0] * G.nb[1]);
}

// Stage 1.  The brick's corner lattice spans [lo, hi] per axis; c = its centre,
// R = its half-diagonal.  map() is 1-Lipschitz up to the rotation constants'
// rounding (x(1 + 2^-16)), so every corner value lies within
// R (1 + 2^-16) of the centre's, up to the f32 error of the evaluations and of
// the point arithmetic: a few tens of ulp of |p|_1 + |d| + bound_k, for which
// mg = 2^-10 (|c|_1 + R + |d_c| + bound_k) stands, as in tap_bound.  Beyond that
// distance from iso every corner is on the centre's side and finite: no
// active cell, no void cell, no sign-changing edge.
__global__ __launch_bounds__(256) void mesh_skip_kernel(PtMeshScene S, PtMeshGrid G, PtMeshBufs B, int skip) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= G.n_bricks) return;
    uint32_t evaluate = 1u;
    if (skip && __builtin_isfinite(S.bound_k)) {
        uint32_t bc[3];
        brick_coords(G, b, bc);
        float c[3], r2 = 0.0f;
        for (int a = 0; a < 3; ++a) {
            const uint32_t i0 = bc[a] * PT_MESH_BRICK;
            const uint32_t i1 = i0 + PT_MESH_BRICK < G.n[a] ? i0 + PT_MESH_BRICK : G.n[a];
            const float lo = corner_pos(G, a, i0), hi = corner_pos(G, a, i1);
            c[a] = (lo + hi) * 0.5f;
            r2 += (hi - lo) * (hi - lo);
        }
        const float R = 0.5f * sqrtf(r2);
        const float dc = mesh_map(S.nodes, S.n_nodes, c[0], c[1], c[2]).d;
        const float mg = 0x1p-10f * (fabsf(c[0]) + fabsf(c[1]) + fabsf(c[2]) + R + fabsf(dc) + S.bound_k);
        // (a NaN anywhere fails the comparison: the brick is evaluated)
        if (__builtin_isfinite(dc) && fabsf(dc - G.iso) > R * 0x1.0001p+0f + mg) evaluate = 0u;
    }
    B.flag[b] = evaluate;
}

// Exclusive prefix sums by one workgroup of 16 waves, a tile of 1024 values at
// a time with a running carry.  MODE 0: out[i] = the sum before i.  MODE 1:
// `in` are the skip stage's flags: out = the brick -> slot table (-1 where the
// flag is 0) and list = its inverse.
template <int MODE>
__global__ __launch_bounds__(1024) void mesh_scan_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                         uint32_t *__restrict__ list, uint32_t n,
                                                         unsigned long long *__restrict__ total) {
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned long long carry = 0ull;
    for (uint32_t base = 0; base < n; base += 1024u) {  // (n is uniform: every thread takes every trip)
        const uint32_t i = base + tid;
        const uint32_t v = i < n ? in[i] : 0u;
        uint32_t s = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(s, off, 64);
            if (int(lane) >= off) s += t;
        }
        if (lane == 63u) wsum[wave] = s;
        __syncthreads();
        uint32_t before = 0u, tile = 0u;
        for (uint32_t w = 0; w < 16u; ++w) {
            const uint32_t x = wsum[w];
            before += w < wave ? x : 0u;
            tile += x;
        }
        const uint32_t excl = uint32_t(carry) + before + (s - v);
        if (i < n) {
            if constexpr (MODE == 0) {
                out[i] = excl;
            } else {
                out[i] = v ? excl : 0xffffffffu;
                if (v) list[excl] = i;
            }
        }
        carry += tile;
        __syncthreads();
    }
    if (tid == 0u) *total = carry;
}

struct BrickGeom {
    uint32_t g0[3];   // global index of the brick's first corner / cell
    uint32_t ext[3];  // cells of the brick per axis (1..8): lattice points 0..ext
};
__device__ __forceinline__ BrickGeom brick_geom(const PtMeshGrid &G, uint32_t b) {
    BrickGeom g;
    uint32_t bc[3];
    brick_coords(G, b, bc);
    for (int a = 0; a < 3; ++a) {
        g.g0[a] = bc[a] * PT_MESH_BRICK;
        const uint32_t left = G.n[a] - g.g0[a];
        g.ext[a] = left < PT_MESH_BRICK ? left : PT_MESH_BRICK;
    }
    return g;
}

__device__ __forceinline__ int lat_index(uint32_t x, uint32_t y, uint32_t z) {
    return int((z * PT_MESH_LAT + y) * PT_MESH_LAT + x);
}

// Stage 2: one workgroup of 512 threads (a thread per cell, a wave per mask word) per evaluated brick
__global__ __launch_bounds__(PT_MESH_CELLS3) void mesh_classify_kernel(PtMeshScene S, PtMeshGrid G, PtMeshBufs B) {
    __shared__ float lat[PT_MESH_LAT3];
    __shared__ uint32_t acc[4];  // clipped edges, void cells, corner evaluations, vertices
    const uint32_t slot = blockIdx.x, tid = threadIdx.x;
    const BrickGeom bg = brick_geom(G, B.list[slot]);
    if (tid < 4u) acc[tid] = 0u;
    // the corner lattice, clipped at the grid's edge (points past it: never read)
    uint32_t evals = 0u;
    for (uint32_t p = tid; p < PT_MESH_LAT3; p += PT_MESH_CELLS3) {
        const uint32_t l[3] = {p % PT_MESH_LAT, (p / PT_MESH_LAT) % PT_MESH_LAT, p / (PT_MESH_LAT * PT_MESH_LAT)};
        float d = __builtin_inff();
        if (l[0] <= bg.ext[0] && l[1] <= bg.ext[1] && l[2] <= bg.ext[2]) {
            d = mesh_map(S.nodes, S.n_nodes, corner_pos(G, 0, bg.g0[0] + l[0]), corner_pos(G, 1, bg.g0[1] + l[1]),
                         corner_pos(G, 2, bg.g0[2] + l[2])).d;
            ++evals;
        }
        lat[p] = d;
        B.lattice[size_t(slot) * PT_MESH_LAT3 + p] = d;
    }
    __syncthreads();
    // sign-changing edges on the grid's boundary: each lattice edge is counted by the one brick that owns
    // its lower endpoint (a point on the brick's far face belongs to the next brick, unless the grid ends there)
    uint32_t clipped = 0u;
    for (uint32_t p = tid; p < PT_MESH_LAT3; p += PT_MESH_CELLS3) {
        const uint32_t l[3] = {p % PT_MESH_LAT, (p / PT_MESH_LAT) % PT_MESH_LAT, p / (PT_MESH_LAT * PT_MESH_LAT)};
        if (!(l[0] <= bg.ext[0] && l[1] <= bg.ext[1] && l[2] <= bg.ext[2])) continue;
        const bool in0 = lat[p] < G.iso;
        for (int a = 0; a < 3; ++a) {
            const int u = (a + 1) % 3, v = (a + 2) % 3;
            if (l[a] >= bg.ext[a]) continue;  // no edge along a from here inside the grid
            const uint32_t gu = bg.g0[u] + l[u], gv = bg.g0[v] + l[v];
            const bool owned = (l[u] < PT_MESH_BRICK || gu == G.n[u]) && (l[v] < PT_MESH_BRICK || gv == G.n[v]);
            const bool boundary = gu == 0u || gu == G.n[u] || gv == 0u || gv == G.n[v];
            if (!owned || !boundary) continue;
            uint32_t q[3] = {l[0], l[1], l[2]};
            ++q[a];
            if ((lat[lat_index(q[0], q[1], q[2])] < G.iso) != in0) ++clipped;
        }
    }
    // the cells
    const uint32_t lx = tid & 7u, ly = (tid >> 3) & 7u, lz = tid >> 6;
    const bool valid = lx < bg.ext[0] && ly < bg.ext[1] && lz < bg.ext[2];
    bool has_vertex = false, is_void = false, edge[3] = {false, false, false};
    if (valid) {
        int inside = 0;
        bool finite = true;
        for (int k = 0; k < 8; ++k) {
            const float d = lat[lat_index(lx + (k & 1), ly + ((k >> 1) & 1), lz + (k >> 2))];
            inside += d < G.iso ? 1 : 0;
            finite = finite && __builtin_isfinite(d);
        }
        is_void = !finite;
        has_vertex = finite && inside != 0 && inside != 8;
        const bool in0 = lat[lat_index(lx, ly, lz)] < G.iso;
        edge[0] = (lat[lat_index(lx + 1, ly, lz)] < G.iso) != in0;
        edge[1] = (lat[lat_index(lx, ly + 1, lz)] < G.iso) != in0;
        edge[2] = (lat[lat_index(lx, ly, lz + 1)] < G.iso) != in0;
    }
    const uint64_t vm = __ballot(has_vertex), voids = __ballot(is_void);
    const uint64_t e0 = __ballot(edge[0]), e1 = __ballot(edge[1]), e2 = __ballot(edge[2]);
    const uint32_t wave = tid >> 6;
    if ((tid & 63u) == 0u) {
        B.vmask[size_t(slot) * PT_MESH_WORDS + wave] = vm;
        uint64_t *q = B.qmask + size_t(slot) * 3 * PT_MESH_WORDS;
        q[wave] = e0;
        q[PT_MESH_WORDS + wave] = e1;
        q[2 * PT_MESH_WORDS + wave] = e2;
        atomicAdd(&acc[1], uint32_t(__popcll(voids)));
        atomicAdd(&acc[3], uint32_t(__popcll(vm)));
    }
    if (clipped) atomicAdd(&acc[0], clipped);
    if (evals) atomicAdd(&acc[2], evals);
    __syncthreads();
    if (tid == 0u) {
        B.nv[slot] = acc[3];
        if (acc[0]) atomicAdd(&B.ctr[PT_MC_CLIPPED], (unsigned long long)acc[0]);
        if (acc[1]) atomicAdd(&B.ctr[PT_MC_VOID], (unsigned long long)acc[1]);
        atomicAdd(&B.ctr[PT_MC_EVALS], (unsigned long long)acc[2]);
    }
}

// Does cell (c[0], c[1], c[2]) (inside the grid) have a vertex, and which?  Its
// brick's slot from the dense table, its bit in that slot's mask; the index is
// the brick's base plus the mask bits below it.
__device__ __forceinline__ bool cell_vertex(const PtMeshGrid &G, const PtMeshBufs &B, const uint32_t c[3], bool want_index,
                                            uint32_t &index) {
    const uint32_t b = ((c[2] / PT_MESH_BRICK) * G.nb[1] + c[1] / PT_MESH_BRICK) * G.nb[0] + c[0] / PT_MESH_BRICK;
    const int32_t slot = B.slot[b];
    if (slot < 0) return false;
    const uint32_t local = ((c[2] % PT_MESH_BRICK) * PT_MESH_BRICK + c[1] % PT_MESH_BRICK) * PT_MESH_BRICK +
                           c[0] % PT_MESH_BRICK;
    const uint64_t *m = B.vmask + size_t(slot) * PT_MESH_WORDS;
    const uint32_t w = local >> 6;
    const uint64_t word = m[w];
    if (!((word >> (local & 63u)) & 1ull)) return false;
    if (want_index) {
        uint32_t below = uint32_t(__popcll(word & ((1ull << (local & 63u)) - 1ull)));
        for (uint32_t k = 0; k < w; ++k) below += uint32_t(__popcll(m[k]));
        index = B.vbase[slot] + below;
    }
    return true;
}

// the four cells around the axis-a edge whose lower endpoint is corner g (= cell g), in quad order:
// (du, dv) = (-1, -1), (0, -1), (0, 0), (-1, 0) with u = (a + 1) % 3, v = (a + 2) % 3
__device__ __forceinline__ void quad_cell(const uint32_t g[3], int a, int k, uint32_t c[3]) {
    const int u = (a + 1) % 3, v = (a + 2) % 3;
    c[0] = g[0];
    c[1] = g[1];
    c[2] = g[2];
    if (k == 0 || k == 3) --c[u];
    if (k == 0 || k == 1) --c[v];
}

// Stage 2b: of the sign-changing edges, those that emit a quad.  An edge with a
// lower endpoint coordinate 0 across it lies on the grid's boundary (classify
// counted it); next to a cell without a vertex (a void cell) the quad is dropped.
__global__ __launch_bounds__(PT_MESH_CELLS3) void mesh_count_kernel(PtMeshGrid G, PtMeshBufs B) {
    __shared__ uint32_t acc[2];  // triangles, dropped quads
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const BrickGeom bg = brick_geom(G, B.list[slot]);
    if (tid < 2u) acc[tid] = 0u;
    __syncthreads();
    uint64_t *q = B.qmask + size_t(slot) * 3 * PT_MESH_WORDS;
    const uint32_t g[3] = {bg.g0[0] + (tid & 7u), bg.g0[1] + ((tid >> 3) & 7u), bg.g0[2] + (tid >> 6)};
    uint32_t quads = 0u, dropped = 0u;
    for (int a = 0; a < 3; ++a) {
        const int u = (a + 1) % 3, v = (a + 2) % 3;
        const bool crossing = ((q[a * PT_MESH_WORDS + wave] >> lane) & 1ull) != 0;  // (set only for cells inside the grid)
        bool emit = false;
        if (crossing && g[u] >= 1u && g[v] >= 1u) {
            emit = true;
            for (int k = 0; k < 4; ++k) {
                uint32_t c[3], unused;
                quad_cell(g, a, k, c);
                emit = cell_vertex(G, B, c, false, unused) && emit;
            }
            if (!emit) ++dropped;
        }
        const uint64_t em = __ballot(emit);
        if (lane == 0u) q[a * PT_MESH_WORDS + wave] = em;  // (this wave's own word: no other wave or brick reads it here)
        quads += emit ? 1u : 0u;
    }
    if (quads) atomicAdd(&acc[0], 2u * quads);
    if (dropped) atomicAdd(&acc[1], dropped);
    __syncthreads();
    if (tid == 0u) {
        B.nt[slot] = acc[0];
        if (acc[1]) atomicAdd(&B.ctr[PT_MC_DROPPED], (unsigned long long)acc[1]);
    }
}

// Stage 4b: one thread per vertex, so the waves that run map() are full (a brick's
// 512 cells hold some 34 vertices): the crossing mean from the cell's 8 corner
// values, the projection steps, the normal and the shape
__global__ __launch_bounds__(256) void mesh_vertex_kernel(PtMeshScene S, PtMeshGrid G, PtMeshBufs B, uint32_t n_vertices) {
    const uint32_t vi = blockIdx.x * 256u + threadIdx.x;
    if (vi >= n_vertices) return;
    const uint32_t cell = B.vcell[vi], slot = cell / PT_MESH_CELLS3, local = cell % PT_MESH_CELLS3;
    const BrickGeom bg = brick_geom(G, B.list[slot]);
    const float *lat = B.lattice + size_t(slot) * PT_MESH_LAT3;
    const uint32_t l[3] = {local & 7u, (local >> 3) & 7u, local >> 6};
    const uint32_t g[3] = {bg.g0[0] + l[0], bg.g0[1] + l[1], bg.g0[2] + l[2]};
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = corner_pos(G, a, g[a]);
        hi[a] = corner_pos(G, a, g[a] + 1u);
    }
    // the mean of the crossings: x-edges at (j, k) = (0,0), (1,0), (0,1), (1,1), then the y-, then the z-edges
    float sum[3] = {0.0f, 0.0f, 0.0f};
    int count = 0;
    for (int a = 0; a < 3; ++a) {
        const int u = (a + 1) % 3, v = (a + 2) % 3;
        for (int e = 0; e < 4; ++e) {
            uint32_t ca[3] = {l[0], l[1], l[2]};
            ca[u] += uint32_t(e & 1);
            ca[v] += uint32_t(e >> 1);
            uint32_t cb[3] = {ca[0], ca[1], ca[2]};
            ++cb[a];
            const float dA = lat[lat_index(ca[0], ca[1], ca[2])], dB = lat[lat_index(cb[0], cb[1], cb[2])];
            if ((dA < G.iso) == (dB < G.iso)) continue;
            const float t = (G.iso - dA) / (dB - dA);
            float q[3];
            q[u] = (e & 1) ? hi[u] : lo[u];
            q[v] = (e >> 1) ? hi[v] : lo[v];
            q[a] = lo[a] + (hi[a] - lo[a]) * t;
            sum[0] += q[0];
            sum[1] += q[1];
            sum[2] += q[2];
            ++count;
        }
    }
    const float fc = float(count);
    pt_f3 p{sum[0] / fc, sum[1] / fc, sum[2] / fc};
    // projection: p' = p - n (map(p) - iso), clamped into the cell; the last trip takes the attributes
    for (uint32_t step = 0;; ++step) {
        const Hit h = mesh_map(S.nodes, S.n_nodes, p.x, p.y, p.z);
        const pt_f3 n = mesh_normal(S.nodes, S.n_nodes, p);
        if (step >= G.project) {
            B.pos[3 * size_t(vi)] = p.x;
            B.pos[3 * size_t(vi) + 1] = p.y;
            B.pos[3 * size_t(vi) + 2] = p.z;
            B.nrm[3 * size_t(vi)] = n.x;
            B.nrm[3 * size_t(vi) + 1] = n.y;
            B.nrm[3 * size_t(vi) + 2] = n.z;
            B.shp[vi] = h.m - 1;
            break;
        }
        const float d = h.d - G.iso;
        const float qx = p.x - n.x * d, qy = p.y - n.y * d, qz = p.z - n.z * d;
        if (__builtin_isfinite(qx) && __builtin_isfinite(qy) && __builtin_isfinite(qz)) {
            p.x = pt_gmin(pt_gmax(qx, lo[0]), hi[0]);
            p.y = pt_gmin(pt_gmax(qy, lo[1]), hi[1]);
            p.z = pt_gmin(pt_gmax(qz, lo[2]), hi[2]);
        }
    }
}

// Stage 4a: the triangles of one brick, and for each of its vertices the cell it belongs to
__global__ __launch_bounds__(PT_MESH_CELLS3) void mesh_emit_kernel(PtMeshGrid G, PtMeshBufs B) {
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const BrickGeom bg = brick_geom(G, B.list[slot]);
    const float *lat = B.lattice + size_t(slot) * PT_MESH_LAT3;
    const uint32_t l[3] = {tid & 7u, (tid >> 3) & 7u, tid >> 6};
    const uint32_t g[3] = {bg.g0[0] + l[0], bg.g0[1] + l[1], bg.g0[2] + l[2]};
    const uint64_t *vm = B.vmask + size_t(slot) * PT_MESH_WORDS;
    const uint64_t *qm = B.qmask + size_t(slot) * 3 * PT_MESH_WORDS;
    const uint64_t below = (1ull << lane) - 1ull;
    // ---- the vertex: its index from the mask, its cell for stage 4b ----
    if ((vm[wave] >> lane) & 1ull) {
        uint32_t vi = B.vbase[slot] + uint32_t(__popcll(vm[wave] & below));
        for (uint32_t w = 0; w < wave; ++w) vi += uint32_t(__popcll(vm[w]));
        B.vcell[vi] = slot * PT_MESH_CELLS3 + tid;  // (slot < 2^21: 30 bits)
    }
    // ---- the triangles: by cell, then by axis ----
    const uint32_t mine = uint32_t((qm[wave] >> lane) & 1ull) | uint32_t((qm[PT_MESH_WORDS + wave] >> lane) & 1ull) << 1 |
                          uint32_t((qm[2 * PT_MESH_WORDS + wave] >> lane) & 1ull) << 2;
    if (!mine) return;
    uint32_t quads_before = 0u;
    for (int a = 0; a < 3; ++a) {
        quads_before += uint32_t(__popcll(qm[a * PT_MESH_WORDS + wave] & below));
        for (uint32_t w = 0; w < wave; ++w) quads_before += uint32_t(__popcll(qm[a * PT_MESH_WORDS + w]));
    }
    size_t t = size_t(B.tbase[slot]) + 2u * size_t(quads_before);
    const bool inside = lat[lat_index(l[0], l[1], l[2])] < G.iso;
    for (int a = 0; a < 3; ++a) {
        if (!((mine >> a) & 1u)) continue;
        uint32_t qv[4];
        for (int k = 0; k < 4; ++k) {
            uint32_t c[3];
            quad_cell(g, a, k, c);
            qv[inside ? k : 3 - k] = 0u;
            (void)cell_vertex(G, B, c, true, qv[inside ? k : 3 - k]);  // (the count stage saw all four)
        }
        uint32_t *o = B.tri + 3 * t;
        o[0] = qv[0];
        o[1] = qv[1];
        o[2] = qv[2];
        o[3] = qv[0];
        o[4] = qv[2];
        o[5] = qv[3];
        t += 2;
    }
}

}  // namespace pt

void pt_launch_sample(const PtMeshScene &S, const float *xyz, uint32_t n, float *d, int32_t *shape, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(pt::mesh_sample_kernel, dim3(uint32_t((uint64_t(n) + 255u) / 256u)), dim3(256), 0, stream, S, xyz, n, d, shape);
}

void pt_launch_mesh_skip(const PtMeshScene &S, const PtMeshGrid &G, const PtMeshBufs &B, bool skip, hipStream_t stream) {
    hipLaunchKernelGGL(pt::mesh_skip_kernel, dim3((G.n_bricks + 255u) / 256u), dim3(256), 0, stream, S, G, B, skip ? 1 : 0);
}

void pt_launch_mesh_slots(const PtMeshGrid &G, const PtMeshBufs &B, hipStream_t stream) {
    hipLaunchKernelGGL(pt::mesh_scan_kernel<1>, dim3(1), dim3(1024), 0, stream, B.flag, reinterpret_cast<uint32_t *>(B.slot),
                       B.list, G.n_bricks, B.ctr + PT_MC_SLOTS);
}

void pt_launch_mesh_classify(const PtMeshScene &S, const PtMeshGrid &G, const PtMeshBufs &B, uint32_t n_eval,
                             hipStream_t stream) {
    if (!n_eval) return;
    hipLaunchKernelGGL(pt::mesh_classify_kernel, dim3(n_eval), dim3(PT_MESH_CELLS3), 0, stream, S, G, B);
}

void pt_launch_mesh_count(const PtMeshGrid &G, const PtMeshBufs &B, uint32_t n_eval, hipStream_t stream) {
    if (!n_eval) return;
    hipLaunchKernelGGL(pt::mesh_count_kernel, dim3(n_eval), dim3(PT_MESH_CELLS3), 0, stream, G, B);
}

void pt_launch_mesh_scan(const PtMeshBufs &B, uint32_t n_eval, hipStream_t stream) {
    hipLaunchKernelGGL(pt::mesh_scan_kernel<0>, dim3(1), dim3(1024), 0, stream, B.nv, B.vbase, (uint32_t *)nullptr, n_eval,
                       B.ctr + PT_MC_VERTS);
    hipLaunchKernelGGL(pt::mesh_scan_kernel<0>, dim3(1), dim3(1024), 0, stream, B.nt, B.tbase, (uint32_t *)nullptr, n_eval,
                       B.ctr + PT_MC_TRIS);
}

void pt_launch_mesh_emit(const PtMeshScene &S, const PtMeshGrid &G, const PtMeshBufs &B, uint32_t n_eval,
                         uint32_t n_vertices, hipStream_t stream) {
    if (!n_eval) return;
    hipLaunchKernelGGL(pt::mesh_emit_kernel, dim3(n_eval), dim3(PT_MESH_CELLS3), 0, stream, G, B);
    if (n_vertices)
        hipLaunchKernelGGL(pt::mesh_vertex_kernel, dim3((n_vertices + 255u) / 256u), dim3(256), 0, stream, S, G, B, n_vertices);
}
