// pt_mesh.h -- launch parameters of the mesh export kernels (pt_mesh.hip):
// pt_sample_field's one-thread-per-point map() and the surface-nets extractor
// of pt_mesh_extract.  Shared with the host entry points in
// pt_mesh_host.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_device.h"

#define PT_MESH_LAT (PT_MESH_BRICK + 1)                         // corner lattice points per brick edge
#define PT_MESH_LAT3 (PT_MESH_LAT * PT_MESH_LAT * PT_MESH_LAT)  // 729
#define PT_MESH_CELLS3 (PT_MESH_BRICK * PT_MESH_BRICK * PT_MESH_BRICK)  // 512: one thread each, 8 waves
#define PT_MESH_WORDS (PT_MESH_CELLS3 / 64)                     // 64-bit mask words per brick: one per wave

// the scene tables map() reads, and the map() bound's margin constant (pt_bound_k; NaN: no bound)
struct PtMeshScene {
    const PtNode *nodes;
    int32_t n_nodes;
    float bound_k;
};

struct PtMeshGrid {
    float origin[3];
    float cell;
    uint32_t n[3];   // cells per axis
    uint32_t nb[3];  // bricks per axis
    float iso;
    uint32_t project;
    uint32_t n_bricks;
};

// order-free counters of one extract (the only atomics), then the scans' totals
enum { PT_MC_CLIPPED = 0, PT_MC_VOID, PT_MC_DROPPED, PT_MC_EVALS, PT_MC_SLOTS, PT_MC_VERTS, PT_MC_TRIS, PT_MC_COUNT };

struct PtMeshBufs {
    // per brick
    uint32_t *flag;  // 1: evaluate (the skip stage's answer)
    int32_t *slot;   // brick -> slot among the evaluated ones, in brick order; -1: skipped
    // per evaluated brick (slot)
    uint32_t *list;       // slot -> brick
    float *lattice;       // [PT_MESH_LAT3] corner values, (z * 9 + y) * 9 + x
    uint64_t *vmask;      // [PT_MESH_WORDS] cells with a vertex, bit = local cell (lz * 8 + ly) * 8 + lx
    uint64_t *qmask;      // [3][PT_MESH_WORDS] per axis: classify, the cell's edge changes sign; count, it emits a quad
    uint32_t *nv, *nt;    // vertices and triangles of the brick
    uint32_t *vbase, *tbase;  // their exclusive prefix sums
    unsigned long long *ctr;  // [PT_MC_COUNT]
    // the mesh
    float *pos, *nrm;
    int32_t *shp;
    uint32_t *tri;
    uint32_t *vcell;  // per vertex: slot * 512 + local cell (emit -> the per-vertex stage)
};

void pt_launch_sample(const PtMeshScene &S, const float *xyz, uint32_t n, float *d, int32_t *shape, hipStream_t stream);
// the extractor's stages, each its own launch; n_eval: evaluated bricks (the grid of the per-brick stages)
void pt_launch_mesh_skip(const PtMeshScene &S, const PtMeshGrid &G, const PtMeshBufs &B, bool skip, hipStream_t stream);
void pt_launch_mesh_slots(const PtMeshGrid &G, const PtMeshBufs &B, hipStream_t stream);  // flag -> slot, list, ctr[SLOTS]
void pt_launch_mesh_classify(const PtMeshScene &S, const PtMeshGrid &G, const PtMeshBufs &B, uint32_t n_eval,
                             hipStream_t stream);
void pt_launch_mesh_count(const PtMeshGrid &G, const PtMeshBufs &B, uint32_t n_eval, hipStream_t stream);
void pt_launch_mesh_scan(const PtMeshBufs &B, uint32_t n_eval, hipStream_t stream);  // nv, nt -> vbase, tbase, ctr[VERTS, TRIS]
// triangles and the vertices' cells per evaluated brick, then one thread per vertex
void pt_launch_mesh_emit(const PtMeshScene &S, const PtMeshGrid &G, const PtMeshBufs &B, uint32_t n_eval,
                         uint32_t n_vertices, hipStream_t stream);
