// Corrected submaps fused into one voxel map (include/epcnet_maps.h: epcnet_map_fuse; numpy restatement in tests/map_ref.py): the step
// behind the loop closing.  The definition is float64 with every operation rounded once (contract off) up to an integer lattice of
// voxel / 4096, and integers from there on: cells, sums, the mean.  Integer sums do not depend on the order of arrival, so the atomics
// below leave the same bits on every run.
//
// offsets, poses and origin are device data: every grid is sized from num_rows and max_voxels alone.
//   scan_clear_words       clears the workspace's head (scan_common.h: a launch, not a memset)
//   map_clear_kernel       every slot of the table to (empty key, no leader, zero sums); the offsets' rule, an integer OR into the head
//   map_insert_kernel      the hot path.  One thread per row, MP_TILE rows per workgroup: the tile finds the clouds of its first and last
//                          row by binary search ONCE, the pose of the first comes through LDS; transform, classify, key; the claim of a
//                          slot of the open-addressing table (mp_claim), then this file's own integer atomics on the slot, one lane per
//                          row: three sums, the count, atomicMin on the leader.  The slot a row landed in goes to row_slot (negative:
//                          no kept row).  The claimed slots are counted: more than max_voxels is the overflow, and a probe gives up
//                          once it sees that.  (The prologue is surfel_common.h's sf_tile_row written out: as a call it leaves w live
//                          across the helper's end, ten more instructions; DESIGN.md, "What the voxel maps share".)
//   map_count_kernel, map_group_kernel, map_top_kernel      every leader's number: mp_is_leader counted per tile, mp_scan_group, mp_top; num_out
//   map_emit_kernel        tiles over the rows: a leader's j = group + tile + its place in the tile; it writes row j and count j from its
//                          slot.  Behind them tiles over the voxels: NaN rows and zero counts for j >= V, or everywhere after an overflow
//                          or a failed call.
// No float atomics, no inline assembly.  What does not follow the 40-byte slot -- the shape's refusals, key and cell, the claim loop, the
// scan -- is map_common.h's, shared with the surfel files; the slot, its adds and the mean written from it are this file's.
#include "map_common.h"

// one slot of the table: 40 bytes
struct mp_slot {
    unsigned long long key;
    unsigned long long sum[3];
    int32_t cnt;
    int32_t leader;
};

// the workspace: head (16 int32) | table (cap slots) | row_slot (num_rows int32) | tile counts (int32) | group totals (int32)
struct mp_ws {
    int32_t* head;
    mp_slot* table;
    int32_t* row_slot;
    int32_t* tile;
    int32_t* group;
    unsigned long long mask;   // cap - 1
};
// the regions of mp_ws in `workspace`, or (workspace NULL) only their total: the head and the table as they are, the rest rounded up to 16 bytes
struct mp_layout_t { mp_ws ws; size_t bytes; };
static mp_layout_t mp_layout(void* workspace, long long num_rows, long long max_voxels) {
    epc_carver c(workspace);
    const unsigned long long cap = mp_cap(max_voxels);
    return {{c.take<int32_t>(MP_HEAD), c.take<mp_slot>(cap), c.take<int32_t>((size_t)num_rows, 16), c.take<int32_t>((size_t)mp_tiles(num_rows), 16),
             c.take<int32_t>((size_t)mp_groups(num_rows), 16), cap - 1}, c.bytes()};
}

struct mp_params {
    double voxel, step;        // step = fl(voxel / 4096)
    long long min_count;
};

// ---- launch 2: the table, and the whole-call failure -----------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void map_clear_kernel(const int32_t* __restrict__ offsets, long long num_rows, int num_clouds,
                                                               mp_ws ws) {
    const unsigned long long stride = (unsigned long long)gridDim.x * MP_THREADS;
    const unsigned long long first = (unsigned long long)blockIdx.x * MP_THREADS + threadIdx.x;
    for (unsigned long long s = first; s <= ws.mask; s += stride) {
        mp_slot* t = ws.table + s;
        t->key = MP_EMPTY;
        t->sum[0] = 0, t->sum[1] = 0, t->sum[2] = 0;
        t->cnt = 0, t->leader = MP_NO_LEADER;
    }
    bool bad = false;
    const long long checks = num_clouds > 0 ? num_clouds : 1;
    for (long long i = (long long)first; i < checks; i += (long long)stride) bad |= offsets_rule_bad(offsets, num_clouds, num_rows, i);
    if (bad) atomicOr(&ws.head[MP_BAD], 1);
}

// ---- launch 3: the rows ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void map_insert_kernel(const float* __restrict__ points, const int32_t* __restrict__ offsets,
                                                                long long num_rows, int num_clouds, const double* __restrict__ poses,
                                                                const double* __restrict__ origin, mp_params pr, long long max_voxels,
                                                                mp_ws ws) {
    __shared__ double pose_s[12];
    __shared__ int c_first, c_last;
    __shared__ int kinds[3];
    if (ws.head[MP_BAD]) return;                       // (uniform: the launch before this one decided it)
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * MP_TILE, r = r0 + tid;
    const long long r1 = r0 + MP_TILE < num_rows ? r0 + MP_TILE : num_rows;                  // the tile's end
    if (tid == 0) c_first = first_scan_behind(offsets, 0, num_clouds, r0);                   // num_clouds: behind every cloud
    if (tid == 1) c_last = first_scan_behind(offsets, 0, num_clouds, r1 - 1);
    if (tid < 3) kinds[tid] = 0;
    __syncthreads();
    const int cf = c_first, cl = c_last;
    if (tid < 12 && cf < num_clouds) pose_s[tid] = poses[(size_t)cf * 12 + tid];
    __syncthreads();
    int slot = -4;                                     // no row of any cloud
    if (r < num_rows) {
        const int c = cf == cl ? cf : first_scan_behind(offsets, cf, cl, r);
        if (c < num_clouds && r >= (long long)offsets[c]) {
            double m[12], d[3];
            if (c == cf) {
#pragma unroll
                for (int e = 0; e < 12; ++e) m[e] = pose_s[e];
            } else {
#pragma unroll
                for (int e = 0; e < 12; ++e) m[e] = poses[(size_t)c * 12 + e];
            }
            {
#pragma clang fp contract(off)
                d[0] = m[3] - origin[0], d[1] = m[7] - origin[1], d[2] = m[11] - origin[2];
            }
            long long w[3];
            const int kind = mp_row(m, d, pr.voxel, points[(size_t)r * 3], points[(size_t)r * 3 + 1], points[(size_t)r * 3 + 2], w);
            atomicAdd(&kinds[kind], 1);
            slot = -kind;                              // -1 absent, -2 out of range
            if (kind == 0) {
                // (mp_key(w >> 12) written out: as a call its eight instructions come in another order -- DESIGN.md)
                const unsigned long long key = ((unsigned long long)((w[2] >> 12) + EPC_MAP_MAX_CELL) << 42) |
                                               ((unsigned long long)((w[1] >> 12) + EPC_MAP_MAX_CELL) << 21) |
                                               (unsigned long long)((w[0] >> 12) + EPC_MAP_MAX_CELL);
                slot = mp_claim(ws.table, ws.mask, key, &ws.head[MP_CLAIMED], max_voxels);   // -3: gave up
                if (slot >= 0) {
                    mp_slot* t = ws.table + slot;
                    atomicAdd(&t->sum[0], (unsigned long long)(w[0] & 4095));
                    atomicAdd(&t->sum[1], (unsigned long long)(w[1] & 4095));
                    atomicAdd(&t->sum[2], (unsigned long long)(w[2] & 4095));
                    atomicAdd(&t->cnt, 1);
                    if (mp_load(&t->leader) > (int)r) atomicMin(&t->leader, (int)r);      // (it only falls: a stale read costs an atomic)
                }
            }
        }
        ws.row_slot[r] = slot;
    }
    __syncthreads();
    if (tid < 3 && kinds[tid]) atomicAdd(&ws.head[MP_KEPT + tid], kinds[tid]);
}

// ---- launches 4 to 6: every leader's number (map_common.h) -----------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void map_count_kernel(long long num_rows, long long max_voxels, mp_ws ws) {
    __shared__ int part[MP_THREADS / 64];
    if (mp_no_map(ws.head, max_voxels)) return;
    int slot, total;
    block_scan<MP_THREADS / 64, int>(mp_is_leader(ws.table, ws.row_slot, (long long)blockIdx.x * MP_TILE + threadIdx.x, num_rows, &slot), part, total);
    if (threadIdx.x == 0) ws.tile[blockIdx.x] = total;
}

__global__ __launch_bounds__(MP_GROUP) void map_group_kernel(long long tiles, long long max_voxels, mp_ws ws) {
    __shared__ int part[MP_GROUP / 64];
    if (mp_no_map(ws.head, max_voxels)) return;
    mp_scan_group(tiles, ws.tile, ws.group, part);
}

__global__ __launch_bounds__(MP_THREADS) void map_top_kernel(long long groups, long long max_voxels, mp_ws ws, int32_t* __restrict__ num_out) {
    __shared__ int part[MP_THREADS / 64];
    mp_top(ws.head, groups, ws.group, max_voxels, num_out, part);
}

// ---- launch 7: the outputs -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void map_emit_kernel(long long num_rows, long long row_tiles, long long max_voxels, mp_params pr,
                                                              mp_ws ws, float* __restrict__ map_points, int32_t* __restrict__ count) {
    __shared__ int part[MP_THREADS / 64];
    const bool none = mp_no_map(ws.head, max_voxels);  // (uniform)
    const float nan = epc_nan_f32();
    if ((long long)blockIdx.x >= row_tiles) {          // the voxels no leader writes
        const long long j = ((long long)blockIdx.x - row_tiles) * MP_THREADS + threadIdx.x;
        if (j < max_voxels && (none || j >= (long long)ws.head[MP_CLAIMED])) {
            map_points[(size_t)j * 3] = nan, map_points[(size_t)j * 3 + 1] = nan, map_points[(size_t)j * 3 + 2] = nan;
            count[j] = 0;
        }
        return;
    }
    if (none) return;
    int slot = -1, total;
    const int lead = mp_is_leader(ws.table, ws.row_slot, (long long)blockIdx.x * MP_TILE + threadIdx.x, num_rows, &slot);
    const long long j = (long long)ws.group[blockIdx.x / MP_GROUP] + ws.tile[blockIdx.x] + block_scan<MP_THREADS / 64, int>(lead, part, total);
    if (!lead || j >= max_voxels) return;              // (j < V <= max_voxels here: the bound only keeps a wrong number inside the buffers)
    const mp_slot* t = ws.table + slot;
    const long long cnt = t->cnt;
    long long cell[3];
    mp_cell(t->key, cell[0], cell[1], cell[2]);
    float o[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma clang fp contract(off)
        const long long g = cell[a];
        const long long mean = (long long)(t->sum[a] / (unsigned long long)cnt);
        o[a] = cnt >= pr.min_count ? (float)((double)(g * 4096 + mean) * pr.step) : nan;
    }
    map_points[(size_t)j * 3] = o[0], map_points[(size_t)j * 3 + 1] = o[1], map_points[(size_t)j * 3 + 2] = o[2];
    count[j] = (int32_t)cnt;
}

extern "C" size_t epcnet_map_fuse_workspace_bytes(long long num_rows, int num_clouds, long long max_voxels) {
    if (!mp_supported(num_rows, num_clouds, max_voxels)) return 0;
    return mp_layout(nullptr, num_rows, max_voxels).bytes;
}

extern "C" int epcnet_map_fuse(const float* points, const int32_t* offsets, long long num_rows, int num_clouds, const double* poses,
                               const double* origin, const double* params, long long max_voxels, float* map_points, int32_t* count,
                               int32_t* num_out, void* workspace, size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG(points && offsets && poses && origin && params && map_points && count && num_out && workspace, "null pointer");
    const char* const shape = mp_shape_refusal(num_rows, num_clouds, max_voxels);
    EPC_CHECK_ARG(!shape, shape);
    const double voxel = params[0], min_count = params[1];
    EPC_CHECK_ARG(__builtin_isfinite(voxel) && voxel >= 1.0 / 1048576.0 && voxel <= 1048576.0, "voxel must be finite and in [2^-20, 2^20]");
    EPC_CHECK_ARG(min_count >= 1.0 && min_count < 2147483648.0 && min_count == __builtin_floor(min_count),
                  "min_count must be an integer value in [1, 2^31)");
    for (int i = 2; i < EPC_MAP_PARAMS; ++i) EPC_CHECK_ARG(params[i] == 0.0, "the six reserved parameters must be 0");
    EPC_CHECK_WORKSPACE(workspace, workspace_bytes, epcnet_map_fuse_workspace_bytes(num_rows, num_clouds, max_voxels));
    mp_params pr;
    pr.voxel = voxel;
    pr.step = voxel / 4096.0;
    pr.min_count = (long long)min_count;
    hipStream_t st = (hipStream_t)stream;
    const mp_ws ws = mp_layout(workspace, num_rows, max_voxels).ws;
    const long long tiles = mp_tiles(num_rows), groups = mp_groups(num_rows);
    if (int rc = scan_clear_words_launch(ws.head, MP_HEAD, st, __func__)) return rc;
    const unsigned long long clear_blocks = (ws.mask + MP_THREADS) / MP_THREADS;             // cap / MP_THREADS, at least 1
    hipLaunchKernelGGL(map_clear_kernel, dim3((unsigned)(clear_blocks < 65536 ? clear_blocks : 65536)), dim3(MP_THREADS), 0, st, offsets,
                       num_rows, num_clouds, ws);
    EPC_CHECK_LAUNCH();
    if (tiles > 0) {
        hipLaunchKernelGGL(map_insert_kernel, dim3((unsigned)tiles), dim3(MP_THREADS), 0, st, points, offsets, num_rows, num_clouds, poses,
                           origin, pr, max_voxels, ws);
        EPC_CHECK_LAUNCH();
        hipLaunchKernelGGL(map_count_kernel, dim3((unsigned)tiles), dim3(MP_THREADS), 0, st, num_rows, max_voxels, ws);
        EPC_CHECK_LAUNCH();
        hipLaunchKernelGGL(map_group_kernel, dim3((unsigned)groups), dim3(MP_GROUP), 0, st, tiles, max_voxels, ws);
        EPC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(map_top_kernel, dim3(1), dim3(MP_THREADS), 0, st, groups, max_voxels, ws, num_out);
    EPC_CHECK_LAUNCH();
    const long long fill_tiles = (max_voxels + MP_THREADS - 1) / MP_THREADS;
    hipLaunchKernelGGL(map_emit_kernel, dim3((unsigned)(tiles + fill_tiles)), dim3(MP_THREADS), 0, st, num_rows, tiles, max_voxels, pr, ws,
                       map_points, count);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}
