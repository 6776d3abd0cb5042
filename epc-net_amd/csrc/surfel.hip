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
// No float atomics, no inline assembly, no scratch.
#include "map_common.h"
#include "../../include/epcnet_surfels.h"

// one slot of the table: sixteen 64-bit words, 128 bytes
struct sf_slot {
    unsigned long long key;
    unsigned long long cnt;
    unsigned long long sum[3];     // of w_a & 4095: the mean of map_points
    unsigned long long A[3];       // of u_a = (w_a & 4095) >> 4
    unsigned long long B[6];       // of u_a u_b: 00 01 02 11 12 22
    int32_t leader;
    int32_t pad;
    unsigned long long spare;
};
static_assert(sizeof(sf_slot) == 128, "a slot is sixteen 64-bit words");

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

struct sf_params {
    double voxel, step, step8;     // step = fl(voxel / 4096), step8 = fl(voxel / 256)
    long long min_count, min_support;
    int ring;
};

// ---- launch 2: the table, and the whole-call failure -----------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void surfel_clear_kernel(const int32_t* __restrict__ offsets, long long num_rows, int num_clouds,
                                                                  sf_ws ws) {
    const unsigned long long stride = (unsigned long long)gridDim.x * MP_THREADS;
    const unsigned long long first = (unsigned long long)blockIdx.x * MP_THREADS + threadIdx.x;
    // sixteen lanes per slot, one word each: a wave-instruction stores four whole slots
    const unsigned long long words = (ws.mask + 1) * 16;
    unsigned long long* const base = reinterpret_cast<unsigned long long*>(ws.table);
    for (unsigned long long i = first; i < words; i += stride) {
        const unsigned e = (unsigned)(i & 15);
        base[i] = e == 0 ? MP_EMPTY : e == 14 ? (unsigned long long)MP_NO_LEADER : 0ull;      // (word 14: leader in the low half, pad 0)
    }
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
    __shared__ double pose_s[12];
    __shared__ int c_first, c_last;
    __shared__ int kinds[3];
    __shared__ int slot_s[MP_TILE];                    // the slot of every row of the tile, negative: nothing to add
    __shared__ unsigned short pos_s[MP_TILE][4];       // its w_a & 4095
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
                const unsigned long long key = mp_key(w[0] >> 12, w[1] >> 12, w[2] >> 12);
                unsigned long long s = mp_hash(key) & ws.mask;
                slot = -3;                             // gave up: the table overflowed
                for (unsigned probes = 0;; ++probes) {
                    // (a full table holds no empty slot: the count of claimed slots is what ends the walk)
                    if ((probes & 7) == 0 && (long long)mp_load(&ws.head[MP_CLAIMED]) > max_voxels) break;
                    unsigned long long* kp = &ws.table[s].key;
                    unsigned long long k = __atomic_load_n(kp, __ATOMIC_RELAXED);
                    if (k == MP_EMPTY) {
                        k = atomicCAS(kp, MP_EMPTY, key);
                        if (k == MP_EMPTY) {
                            atomicAdd(&ws.head[MP_CLAIMED], 1);
                            k = key;
                        }
                    }
                    if (k == key) {
                        slot = (int)s;
                        break;
                    }
                    s = (s + 1) & ws.mask;
                }
                if (slot >= 0) {
                    pos_s[tid][0] = (unsigned short)(w[0] & 4095), pos_s[tid][1] = (unsigned short)(w[1] & 4095);
                    pos_s[tid][2] = (unsigned short)(w[2] & 4095);
                    int32_t* lead = &ws.table[slot].leader;
                    if (mp_load(lead) > (int)r) atomicMin(lead, (int)r);        // (it only falls: a stale read costs an atomic)
                }
            }
        }
        ws.row_slot[r] = slot;
    }
    slot_s[tid] = slot;
    __syncthreads();
    // sixteen lanes per row, one per word of its slot (1 the count, 2..4 the 12-bit sums, 5..7 A, 8..13 B; the key's, the leader's and the
    // spare lane idle): a wave-instruction adds to four slots of 104 contiguous bytes each
    const int word = tid & 15;
    for (int it = 0; it < MP_TILE / 16; ++it) {
        const int row = it * 16 + (tid >> 4);
        const int sl = slot_s[row];
        if (sl >= 0 && word >= 1 && word <= 13) {
            const unsigned long long p0 = pos_s[row][0], p1 = pos_s[row][1], p2 = pos_s[row][2];
            const unsigned long long u0 = p0 >> 4, u1 = p1 >> 4, u2 = p2 >> 4;
            const unsigned long long x = word < 8 ? (word == 1 || word == 2 || word == 5 ? (word == 1 ? 1ull : word == 2 ? p0 : u0)
                                                                                         : (word == 3 ? p1 : word == 4 ? p2 : word == 6 ? u1 : u2))
                                                  : (word < 11 ? u0 : word < 13 ? u1 : u2);
            const unsigned long long y = word < 8 ? 1ull : (word == 8 ? u0 : word == 9 || word == 11 ? u1 : u2);
            atomicAdd(reinterpret_cast<unsigned long long*>(ws.table + sl) + word, x * y);
        }
    }
    __syncthreads();
    if (tid < 3 && kinds[tid]) atomicAdd(&ws.head[MP_KEPT + tid], kinds[tid]);
}

// the call has no map: the offsets were not valid, or more voxels than max_voxels were claimed (row_slot and the table may not be followed)
__device__ __forceinline__ bool sf_no_map(const sf_ws& ws, long long max_voxels) {
    return ws.head[MP_BAD] != 0 || (long long)ws.head[MP_CLAIMED] > max_voxels;
}

__device__ __forceinline__ int sf_is_leader(const sf_ws& ws, long long r, long long num_rows, int* slot) {
    if (r >= num_rows) return 0;
    const int s = ws.row_slot[r];
    *slot = s;
    return s >= 0 && ws.table[s].leader == (int)r ? 1 : 0;
}

// ---- launches 4 to 6: every leader's number ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void surfel_count_kernel(long long num_rows, long long max_voxels, sf_ws ws) {
    __shared__ int part[MP_THREADS / 64];
    if (sf_no_map(ws, max_voxels)) return;
    int slot, total;
    block_scan<MP_THREADS / 64, int>(sf_is_leader(ws, (long long)blockIdx.x * MP_TILE + threadIdx.x, num_rows, &slot), part, total);
    if (threadIdx.x == 0) ws.tile[blockIdx.x] = total;
}

__global__ __launch_bounds__(MP_GROUP) void surfel_group_kernel(long long tiles, long long max_voxels, sf_ws ws) {
    __shared__ int part[MP_GROUP / 64];
    if (sf_no_map(ws, max_voxels)) return;
    const long long t = (long long)blockIdx.x * MP_GROUP + threadIdx.x;
    const int v = t < tiles ? ws.tile[t] : 0;
    int total;
    const int excl = block_scan<MP_GROUP / 64, int>(v, part, total);
    if (t < tiles) ws.tile[t] = excl;
    if (threadIdx.x == 0) ws.group[blockIdx.x] = total;
}

__global__ __launch_bounds__(MP_THREADS) void surfel_top_kernel(long long groups, long long max_voxels, sf_ws ws, int32_t* __restrict__ num_out) {
    __shared__ int part[MP_THREADS / 64];
    const bool bad = ws.head[MP_BAD] != 0, none = sf_no_map(ws, max_voxels);
    if (!none) {
        int carry = 0;
        for (long long base = 0; base < groups; base += MP_THREADS) {
            const long long g = base + threadIdx.x;
            const int v = g < groups ? ws.group[g] : 0;
            int total;
            const int excl = carry + block_scan<MP_THREADS / 64, int>(v, part, total);
            if (g < groups) ws.group[g] = excl;
            carry += total;
        }
    }
    if (threadIdx.x == 0) {
        num_out[0] = none ? -1 : ws.head[MP_CLAIMED];                       // V: every claimed slot has a leader
        num_out[1] = bad ? 0 : ws.head[MP_KEPT];
        num_out[2] = bad ? 0 : ws.head[MP_KEPT + 1];
        num_out[3] = bad ? 0 : ws.head[MP_KEPT + 2];
    }
}

// ---- launch 7: the outputs -----------------------------------------------------------------------------------------------------------------
// the slot of `key`, or -1: the walk ends at the key or at an empty slot (the table is at most half full)
__device__ __forceinline__ long long sf_find(const sf_ws& ws, unsigned long long key) {
    unsigned long long s = mp_hash(key) & ws.mask;
    for (;;) {
        const unsigned long long k = ws.table[s].key;
        if (k == key) return (long long)s;
        if (k == MP_EMPTY) return -1;
        s = (s + 1) & ws.mask;
    }
}

// one Jacobi rotation of the pair (p, q), r the third index: epcnet_surfels.h
__device__ __forceinline__ void sf_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                          double& v1p, double& v1q, double& v2p, double& v2q) {
#pragma clang fp contract(off)
    const double a = apq;
    if (a == 0.0) return;
    const double theta = (aqq - app) / (2.0 * a);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + __dsqrt_rn(theta * theta + 1.0));
    const double c = 1.0 / __dsqrt_rn(t * t + 1.0);
    const double s = t * c;
    const double h = t * a;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    double g = arp, f = arq;
    arp = c * g - s * f, arq = s * g + c * f;
    g = v0p, f = v0q;
    v0p = c * g - s * f, v0q = s * g + c * f;
    g = v1p, f = v1q;
    v1p = c * g - s * f, v1q = s * g + c * f;
    g = v2p, f = v2q;
    v2p = c * g - s * f, v2q = s * g + c * f;
}

__device__ __forceinline__ double sf_pick(int k, double x0, double x1, double x2) { return k == 0 ? x0 : k == 1 ? x1 : x2; }

__global__ __launch_bounds__(MP_THREADS) void surfel_emit_kernel(long long num_rows, long long row_tiles, long long max_voxels, sf_params pr,
                                                                 sf_ws ws, float* __restrict__ map_points, int32_t* __restrict__ count,
                                                                 float* __restrict__ centroid, float* __restrict__ normal,
                                                                 float* __restrict__ eigen, int32_t* __restrict__ support) {
    __shared__ int part[MP_THREADS / 64];
    __shared__ int lead_slot[MP_TILE];
    const bool none = sf_no_map(ws, max_voxels);       // (uniform)
    const float nan = epc_nan_f32();
    if ((long long)blockIdx.x >= row_tiles) {          // the voxels no leader writes
        const long long j = ((long long)blockIdx.x - row_tiles) * MP_THREADS + threadIdx.x;
        if (j < max_voxels && (none || j >= (long long)ws.head[MP_CLAIMED])) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                map_points[(size_t)j * 3 + a] = nan, centroid[(size_t)j * 3 + a] = nan;
                normal[(size_t)j * 3 + a] = nan, eigen[(size_t)j * 3 + a] = nan;
            }
            count[j] = 0, support[j] = 0;
        }
        return;
    }
    if (none) return;
    int slot = -1, total;
    const int lead = sf_is_leader(ws, (long long)blockIdx.x * MP_TILE + threadIdx.x, num_rows, &slot);
    const int place = block_scan<MP_THREADS / 64, int>(lead, part, total);
    if (lead) lead_slot[place] = slot;                 // the tile's leaders in row order, packed to the first lanes
    __syncthreads();
    if ((int)threadIdx.x >= total) return;
    const long long j = (long long)ws.group[blockIdx.x / MP_GROUP] + ws.tile[blockIdx.x] + threadIdx.x;
    if (j >= max_voxels) return;                       // (j < V <= max_voxels here: the bound only keeps a wrong number inside the buffers)
    const sf_slot* t = ws.table + lead_slot[threadIdx.x];
    const long long cnt = (long long)t->cnt;
    const unsigned long long key = t->key;
    const long long g0 = (long long)(key & 0x1fffff) - EPC_MAP_MAX_CELL, g1 = (long long)((key >> 21) & 0x1fffff) - EPC_MAP_MAX_CELL,
                    g2 = (long long)((key >> 42) & 0x1fffff) - EPC_MAP_MAX_CELL;
    {
#pragma clang fp contract(off)
        const long long m0 = (long long)(t->sum[0] / (unsigned long long)cnt), m1 = (long long)(t->sum[1] / (unsigned long long)cnt),
                        m2 = (long long)(t->sum[2] / (unsigned long long)cnt);
        const bool keep = cnt >= pr.min_count;
        map_points[(size_t)j * 3] = keep ? (float)((double)(g0 * 4096 + m0) * pr.step) : nan;
        map_points[(size_t)j * 3 + 1] = keep ? (float)((double)(g1 * 4096 + m1) * pr.step) : nan;
        map_points[(size_t)j * 3 + 2] = keep ? (float)((double)(g2 * 4096 + m2) * pr.step) : nan;
        count[j] = (int32_t)cnt;
    }
    // the pool, in the frame of cell g: int64
    long long N = 0, S1x = 0, S1y = 0, S1z = 0, Sxx = 0, Sxy = 0, Sxz = 0, Syy = 0, Syz = 0, Szz = 0;
    const int ring = pr.ring;
    for (int o2 = -ring; o2 <= ring; ++o2) {
        const long long c2 = g2 + o2;
        if (c2 < -EPC_MAP_MAX_CELL || c2 >= EPC_MAP_MAX_CELL) continue;
        for (int o1 = -ring; o1 <= ring; ++o1) {
            const long long c1 = g1 + o1;
            if (c1 < -EPC_MAP_MAX_CELL || c1 >= EPC_MAP_MAX_CELL) continue;
            for (int o0 = -ring; o0 <= ring; ++o0) {
                const long long c0 = g0 + o0;
                if (c0 < -EPC_MAP_MAX_CELL || c0 >= EPC_MAP_MAX_CELL) continue;
                const long long at = sf_find(ws, mp_key(c0, c1, c2));
                if (at < 0) continue;
                const sf_slot* q = ws.table + at;
                const long long n = (long long)q->cnt;
                if (n < pr.min_count) continue;
                const long long ex = 256 * o0, ey = 256 * o1, ez = 256 * o2;
                const long long Ax = (long long)q->A[0], Ay = (long long)q->A[1], Az = (long long)q->A[2];
                N += n;
                S1x += Ax + n * ex, S1y += Ay + n * ey, S1z += Az + n * ez;
                Sxx += (long long)q->B[0] + 2 * ex * Ax + n * ex * ex;
                Sxy += (long long)q->B[1] + ex * Ay + ey * Ax + n * ex * ey;
                Sxz += (long long)q->B[2] + ex * Az + ez * Ax + n * ex * ez;
                Syy += (long long)q->B[3] + 2 * ey * Ay + n * ey * ey;
                Syz += (long long)q->B[4] + ey * Az + ez * Ay + n * ey * ez;
                Szz += (long long)q->B[5] + 2 * ez * Az + n * ez * ez;
            }
        }
    }
    support[j] = (int32_t)N;
    float oc0 = nan, oc1 = nan, oc2 = nan, on0 = nan, on1 = nan, on2 = nan, oe0 = nan, oe1 = nan, oe2 = nan;
    if (cnt >= pr.min_count && N >= pr.min_support) {
#pragma clang fp contract(off)
        const double dn = (double)N;
        const double mx = (double)S1x / dn, my = (double)S1y / dn, mz = (double)S1z / dn;
        double a00 = (double)Sxx / dn - mx * mx, a01 = (double)Sxy / dn - mx * my, a02 = (double)Sxz / dn - mx * mz;
        double a11 = (double)Syy / dn - my * my, a12 = (double)Syz / dn - my * mz, a22 = (double)Szz / dn - mz * mz;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
        for (int sweep = 0; sweep < EPC_SURFEL_SWEEPS; ++sweep) {
            sf_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);     // (0, 1), r = 2
            sf_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);     // (0, 2), r = 1
            sf_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);     // (1, 2), r = 0
        }
        // ascending, ties to the lower k
        int k0 = 0;
        double l0 = a00;
        if (a11 < l0) k0 = 1, l0 = a11;
        if (a22 < l0) k0 = 2, l0 = a22;
        const double lp = k0 == 0 ? a11 : a00, lq = k0 == 2 ? a11 : a22;
        const bool swap = lq < lp;
        double l1 = swap ? lq : lp, l2 = swap ? lp : lq;
        l0 = l0 < 0.0 ? 0.0 : l0, l1 = l1 < 0.0 ? 0.0 : l1, l2 = l2 < 0.0 ? 0.0 : l2;
        const double c0 = sf_pick(k0, v00, v01, v02), c1 = sf_pick(k0, v10, v11, v12), c2 = sf_pick(k0, v20, v21, v22);
        const double nn = __dsqrt_rn((c0 * c0 + c1 * c1) + c2 * c2);
        double n0 = c0 / nn, n1 = c1 / nn, n2 = c2 / nn;
        double big = n0;
        if (fabs(n1) > fabs(big)) big = n1;
        if (fabs(n2) > fabs(big)) big = n2;
        if (big < 0.0) n0 = -n0, n1 = -n1, n2 = -n2;
        const double s = pr.step8;
        oc0 = (float)(((double)(256 * g0) + mx) * s), oc1 = (float)(((double)(256 * g1) + my) * s), oc2 = (float)(((double)(256 * g2) + mz) * s);
        on0 = (float)n0, on1 = (float)n1, on2 = (float)n2;
        oe0 = (float)((l0 * s) * s), oe1 = (float)((l1 * s) * s), oe2 = (float)((l2 * s) * s);
    }
    centroid[(size_t)j * 3] = oc0, centroid[(size_t)j * 3 + 1] = oc1, centroid[(size_t)j * 3 + 2] = oc2;
    normal[(size_t)j * 3] = on0, normal[(size_t)j * 3 + 1] = on1, normal[(size_t)j * 3 + 2] = on2;
    eigen[(size_t)j * 3] = oe0, eigen[(size_t)j * 3 + 1] = oe1, eigen[(size_t)j * 3 + 2] = oe2;
}

static bool sf_supported(long long num_rows, int num_clouds, long long max_voxels) {
    return num_rows >= 0 && num_rows < 2147483648ll && num_clouds >= 0 && num_clouds <= (1 << 24) && max_voxels >= 1 &&
           max_voxels <= (1ll << 28);
}

extern "C" size_t epcnet_map_surfels_workspace_bytes(long long num_rows, int num_clouds, long long max_voxels) {
    if (!sf_supported(num_rows, num_clouds, max_voxels)) return 0;
    return sf_layout(nullptr, num_rows, max_voxels).bytes;
}

extern "C" int epcnet_map_surfels(const float* points, const int32_t* offsets, long long num_rows, int num_clouds, const double* poses,
                                  const double* origin, const double* params, long long max_voxels, float* map_points, int32_t* count,
                                  float* centroid, float* normal, float* eigen, int32_t* support, int32_t* num_out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG(points && offsets && poses && origin && params && map_points && count && centroid && normal && eigen && support &&
                      num_out && workspace,
                  "null pointer");
    EPC_CHECK_ARG(num_rows >= 0 && num_rows < 2147483648ll, "need 0 <= num_rows < 2^31");
    EPC_CHECK_ARG(num_clouds >= 0 && num_clouds <= (1 << 24), "need 0 <= num_clouds <= 2^24");
    EPC_CHECK_ARG(max_voxels >= 1 && max_voxels <= (1ll << 28), "need 1 <= max_voxels <= 2^28");
    const double voxel = params[0], min_count = params[1], ring = params[2], min_support = params[3];
    EPC_CHECK_ARG(__builtin_isfinite(voxel) && voxel >= 1.0 / 1048576.0 && voxel <= 1048576.0, "voxel must be finite and in [2^-20, 2^20]");
    EPC_CHECK_ARG(min_count >= 1.0 && min_count < 2147483648.0 && min_count == __builtin_floor(min_count),
                  "min_count must be an integer value in [1, 2^31)");
    EPC_CHECK_ARG(ring >= 0.0 && ring <= (double)EPC_SURFEL_MAX_RING && ring == __builtin_floor(ring),
                  "ring must be an integer value in [0, EPC_SURFEL_MAX_RING]");
    EPC_CHECK_ARG(min_support >= 3.0 && min_support < 2147483648.0 && min_support == __builtin_floor(min_support),
                  "min_support must be an integer value in [3, 2^31)");
    for (int i = 4; i < EPC_SURFEL_PARAMS; ++i) EPC_CHECK_ARG(params[i] == 0.0, "the four reserved parameters must be 0");
    EPC_CHECK_WORKSPACE(workspace, workspace_bytes, epcnet_map_surfels_workspace_bytes(num_rows, num_clouds, max_voxels));
    sf_params pr;
    pr.voxel = voxel;
    pr.step = voxel / 4096.0;
    pr.step8 = voxel / 256.0;
    pr.min_count = (long long)min_count;
    pr.min_support = (long long)min_support;
    pr.ring = (int)ring;
    hipStream_t st = (hipStream_t)stream;
    const sf_ws ws = sf_layout(workspace, num_rows, max_voxels).ws;
    const long long tiles = mp_tiles(num_rows), groups = mp_groups(num_rows);
    if (int rc = scan_clear_words_launch(ws.head, MP_HEAD, st, __func__)) return rc;
    const unsigned long long clear_blocks = ((ws.mask + 1) * 16 + MP_THREADS - 1) / MP_THREADS;
    hipLaunchKernelGGL(surfel_clear_kernel, dim3((unsigned)(clear_blocks < 65536 ? clear_blocks : 65536)), dim3(MP_THREADS), 0, st, offsets,
                       num_rows, num_clouds, ws);
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
