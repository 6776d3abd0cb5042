// The voxel map with a surfel per voxel (include/epcnet_surfels.h: epcnet_map_surfels; numpy restatement in tests/surfel_ref.py).  Rows,
// cells, keys, leaders and numbering are map.hip's (map_common.h); besides the three 12-bit sums every slot collects the count and nine
// integer moments of its rows on a lattice of voxel / 256.  The moments and the sums pooled from them over the (2 ring + 1)^3 cells
// around a voxel are integers: free of the order of arrival.  Behind them the covariance, a cyclic Jacobi and the outputs are a fixed
// sequence of float64 operations, each rounded once (contract off).
//
// offsets, poses and origin are device data: every grid is sized from num_rows and max_voxels alone.
//   scan_clear_words       clears the workspace's head (scan_common.h: a launch, not a memset)
//   surfel_clear_kernel    every slot of the table to (empty key, no leader, zero sums); the offsets' rule, an integer OR into the head
//   surfel_insert_kernel   map_insert_kernel with nine more sums: one thread per row up to the claim by a 64-bit atomicCAS (linear probing)
//                          and the atomicMin on the leader.  A slot is sixteen 64-bit words (128 bytes): the key, the count, three 12-bit
//                          sums, three first and six second moments of the 8-bit lattice, the leader, a spare.  The rows' slots and
//                          positions go through LDS and SIXTEEN lanes serve one row, one per word: a wave-instruction of 64-bit atomic
//                          adds covers four slots of contiguous bytes.  Measured against one lane per row with thirteen scattered 8-byte
//                          atomics (all tests passed in both forms): 11.3 against 14.3 ms on 7.84 M rows, 4.80 against 5.88 ms on 3.67 M
//   surfel_count_kernel, surfel_group_kernel, surfel_top_kernel      every leader's number, as in map.hip; num_out
//   surfel_emit_kernel     tiles over the rows: the tile's leaders are packed to its first lanes through LDS (a voxel's solve is long:
//                          lanes of rows that lead nothing would idle through it); lane i takes the tile's i-th leader, writes map_points
//                          and count from its slot, looks up the (2 ring + 1)^3 cells around it (read-only: hash, linear probing until the
//                          key or an empty slot -- cap >= 2 max_voxels + 1 leaves one), pools their moments in int64 and solves in float64
//                          registers.  Behind them tiles over the voxels: NaN / 0 for j >= V, or everywhere after an overflow or a failed
//                          call.
// No float atomics, no inline assembly, no scratch.  The claim loop, the lookup and the scan are map_common.h's (map.hip runs them
// too); the slot, a tile's rows, the sixteen-lane adds and the pool-and-solve are surfel_common.h's: growmap.hip (the map that grows
// across calls) runs the same definitions on a persistent table.
#include "surfel_common.h"

// the workspace: head (16 int32, padded to 128 bytes: a slot is one 128-byte line of an aligned workspace) | table (cap slots) | row_slot (num_rows int32) | tile counts (int32) | group totals (int32)
struct sf_ws {
    int32_t* head;
    sf_slot* table;
    int32_t* row_slot;
    int32_t* tile;
    int32_t* group;
    unsigned long long mask;   // cap - 1
};
// the regions of sf_ws in `workspace`, or (workspace NULL) only their total: the head and the table as they are, the rest rounded up to 16 bytes
struct sf_layout_t { sf_ws ws; size_t bytes; };
static sf_layout_t sf_layout(void* workspace, long long num_rows, long long max_voxels) {
    epc_carver c(workspace);
    const unsigned long long cap = mp_cap(max_voxels);
    return {{c.take<int32_t>(MP_HEAD, 128), c.take<sf_slot>(cap), c.take<int32_t>((size_t)num_rows, 16), c.take<int32_t>((size_t)mp_tiles(num_rows), 16),
             c.take<int32_t>((size_t)mp_groups(num_rows), 16), cap - 1}, c.bytes()};
}

// ---- launch 2: the table, and the whole-call failure -----------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void surfel_clear_kernel(const int32_t* __restrict__ offsets, long long num_rows, int num_clouds,
                                                                  sf_ws ws) {
    const unsigned long long stride = (unsigned long long)gridDim.x * MP_THREADS;
    const unsigned long long first = (unsigned long long)blockIdx.x * MP_THREADS + threadIdx.x;
    sf_clear_table(ws.table, ws.mask, first, stride);
    bool bad = false;
    const long long checks = num_clouds > 0 ? num_clouds : 1;
    for (long long i = (long long)first; i < checks; i += (long long)stride) bad |= offsets_rule_bad(offsets, num_clouds, num_rows, i);
    if (bad) atomicOr(&ws.head[MP_BAD], 1);
}

// ---- launch 3: the rows ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void surfel_insert_kernel(const float* __restrict__ points, const int32_t* __restrict__ offsets,
                                                                   long long num_rows, int num_clouds, const double* __restrict__ poses,
                                                                   const double* __restrict__ origin, sf_params pr, long long max_voxels,
                                                                   sf_ws ws) {
    __shared__ sf_tile_lds lds;
    if (ws.head[MP_BAD]) return;                       // (uniform: the launch before this one decided it)
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * MP_TILE, r = r0 + tid;
    long long w[3];
    const int kind = sf_tile_row(points, offsets, num_rows, num_clouds, poses, origin, pr.voxel, lds, r0, w);
    int slot = -kind;                                  // -1 absent, -2 out of range, -4 no row of any cloud
    if (kind == 0) {
        slot = mp_claim(ws.table, ws.mask, mp_key(w[0] >> 12, w[1] >> 12, w[2] >> 12), &ws.head[MP_CLAIMED], max_voxels);   // -3: gave up
        if (slot >= 0) {
            sf_stage_pos(lds, tid, w);
            sf_lead(ws.table + slot, r);
        }
    }
    if (r < num_rows) ws.row_slot[r] = slot;
    lds.slot[tid] = slot;
    __syncthreads();
    sf_add_rows(ws.table, lds);
    __syncthreads();
    if (tid < 3 && lds.kinds[tid]) atomicAdd(&ws.head[MP_KEPT + tid], lds.kinds[tid]);
}

// ---- launches 4 to 6: every leader's number (map_common.h) -----------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void surfel_count_kernel(long long num_rows, long long max_voxels, sf_ws ws) {
    __shared__ int part[MP_THREADS / 64];
    if (mp_no_map(ws.head, max_voxels)) return;
    int slot, total;
    block_scan<MP_THREADS / 64, int>(mp_is_leader(ws.table, ws.row_slot, (long long)blockIdx.x * MP_TILE + threadIdx.x, num_rows, &slot), part, total);
    if (threadIdx.x == 0) ws.tile[blockIdx.x] = total;
}

__global__ __launch_bounds__(MP_GROUP) void surfel_group_kernel(long long tiles, long long max_voxels, sf_ws ws) {
    __shared__ int part[MP_GROUP / 64];
    if (mp_no_map(ws.head, max_voxels)) return;
    mp_scan_group(tiles, ws.tile, ws.group, part);
}

__global__ __launch_bounds__(MP_THREADS) void surfel_top_kernel(long long groups, long long max_voxels, sf_ws ws, int32_t* __restrict__ num_out) {
    __shared__ int part[MP_THREADS / 64];
    mp_top(ws.head, groups, ws.group, max_voxels, num_out, part);
}

// ---- launch 7: the outputs -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void surfel_emit_kernel(long long num_rows, long long row_tiles, long long max_voxels, sf_params pr,
                                                                 sf_ws ws, float* __restrict__ map_points, int32_t* __restrict__ count,
                                                                 float* __restrict__ centroid, float* __restrict__ normal,
                                                                 float* __restrict__ eigen, int32_t* __restrict__ support) {
    __shared__ int part[MP_THREADS / 64];
    __shared__ int lead_slot[MP_TILE];
    const bool none = mp_no_map(ws.head, max_voxels);  // (uniform)
    if ((long long)blockIdx.x >= row_tiles) {          // the voxels no leader writes
        const long long j = ((long long)blockIdx.x - row_tiles) * MP_THREADS + threadIdx.x;
        if (j < max_voxels && (none || j >= (long long)ws.head[MP_CLAIMED])) sf_write_none(j, map_points, count, centroid, normal, eigen, support);
        return;
    }
    if (none) return;
    int slot = -1, total;
    const int lead = mp_is_leader(ws.table, ws.row_slot, (long long)blockIdx.x * MP_TILE + threadIdx.x, num_rows, &slot);
    const int place = block_scan<MP_THREADS / 64, int>(lead, part, total);
    if (lead) lead_slot[place] = slot;                 // the tile's leaders in row order, packed to the first lanes
    __syncthreads();
    if ((int)threadIdx.x >= total) return;
    const long long j = (long long)ws.group[blockIdx.x / MP_GROUP] + ws.tile[blockIdx.x] + threadIdx.x;
    if (j >= max_voxels) return;                       // (j < V <= max_voxels here: the bound only keeps a wrong number inside the buffers)
    const sf_slot* t = ws.table + lead_slot[threadIdx.x];
    sf_write_mean(t, pr, j, map_points, count);
    sf_write_surfel(ws.table, ws.mask, t, pr, j, centroid, normal, eigen, support);
}

extern "C" size_t epcnet_map_surfels_workspace_bytes(long long num_rows, int num_clouds, long long max_voxels) {
    if (!mp_supported(num_rows, num_clouds, max_voxels)) return 0;
    return sf_layout(nullptr, num_rows, max_voxels).bytes;
}

extern "C" int epcnet_map_surfels(const float* points, const int32_t* offsets, long long num_rows, int num_clouds, const double* poses,
                                  const double* origin, const double* params, long long max_voxels, float* map_points, int32_t* count,
                                  float* centroid, float* normal, float* eigen, int32_t* support, int32_t* num_out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG(points && offsets && poses && origin && params && map_points && count && centroid && normal && eigen && support &&
                      num_out && workspace,
                  "null pointer");
    const char* const shape = mp_shape_refusal(num_rows, num_clouds, max_voxels);
    EPC_CHECK_ARG(!shape, shape);
    const char* const refusal = sf_params_refusal(params);
    EPC_CHECK_ARG(!refusal, refusal);
    EPC_CHECK_WORKSPACE(workspace, workspace_bytes, epcnet_map_surfels_workspace_bytes(num_rows, num_clouds, max_voxels));
    const sf_params pr = sf_params_of(params);
    hipStream_t st = (hipStream_t)stream;
    const sf_ws ws = sf_layout(workspace, num_rows, max_voxels).ws;
    const long long tiles = mp_tiles(num_rows), groups = mp_groups(num_rows);
    if (int rc = scan_clear_words_launch(ws.head, MP_HEAD, st, __func__)) return rc;
    hipLaunchKernelGGL(surfel_clear_kernel, dim3(sf_clear_blocks(ws.mask)), dim3(MP_THREADS), 0, st, offsets, num_rows, num_clouds, ws);
    EPC_CHECK_LAUNCH();
    if (tiles > 0) {
        hipLaunchKernelGGL(surfel_insert_kernel, dim3((unsigned)tiles), dim3(MP_THREADS), 0, st, points, offsets, num_rows, num_clouds, poses,
                           origin, pr, max_voxels, ws);
        EPC_CHECK_LAUNCH();
        hipLaunchKernelGGL(surfel_count_kernel, dim3((unsigned)tiles), dim3(MP_THREADS), 0, st, num_rows, max_voxels, ws);
        EPC_CHECK_LAUNCH();
        hipLaunchKernelGGL(surfel_group_kernel, dim3((unsigned)groups), dim3(MP_GROUP), 0, st, tiles, max_voxels, ws);
        EPC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(surfel_top_kernel, dim3(1), dim3(MP_THREADS), 0, st, groups, max_voxels, ws, num_out);
    EPC_CHECK_LAUNCH();
    const long long fill_tiles = (max_voxels + MP_THREADS - 1) / MP_THREADS;
    hipLaunchKernelGGL(surfel_emit_kernel, dim3((unsigned)(tiles + fill_tiles)), dim3(MP_THREADS), 0, st, num_rows, tiles, max_voxels, pr, ws,
                       map_points, count, centroid, normal, eigen, support);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}
