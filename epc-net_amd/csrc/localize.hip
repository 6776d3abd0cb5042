// Scan-to-map localisation (include/epcnet_localize.h: epcnet_surfel_index, epcnet_scan_localize; numpy restatement in
// tests/localize_ref.py): point-to-plane ICP of Q scans against the surfels of epcnet_map_surfels.  The definition is float32 distances
// to the indexed surfels of 27 cells in one candidate order, float64 residuals and Jacobians, 29 float64 sums in ONE order (adjacent
// pairing over 4096 leaves indexed by the scan's row), an unpivoted 6 x 6 Cholesky and a retraction, every operation rounded once
// (contract off): the same bits on every run and equal to numpy's.
//
// The index, built once per map: head (32 int32: four counts, M, the bits of voxel) | an open-addressing table of 32-byte slots (the
// key of map_common.h, the winner's centroid, the winner's normal: a hit costs ONE aligned 32-byte read and no second gather) | the
// winner's number per slot, used while building.
//   lz_clear_kernel    every word of the index: empty keys, zero words, no winner; the head
//   lz_insert_kernel   one thread per surfel: claims its cell's slot by a 64-bit atomicCAS (linear probing), atomicMin on the winner
//   lz_fill_kernel     one thread per surfel: the winner copies its six words into the slot; the four counts
//   lz_num_kernel      num from the head
// The localisation: scans, seeds and the index are device data, every grid is sized from Q, H and n alone, nothing is read back.
//   lz_prep_kernel     one workgroup per scan: the rows that are not absent, which seeds are finite (or the identity where there are
//                      none), whether the index records this M and voxel; writes the scan's state and the run flags of stage A
//   lz_corr_kernel     the hot path, one per pass.  Grid (scan, seed, chunk of PS_CHUNK rows), one row per lane.  The 27 lookups are
//                      latency-bound (the table is far larger than L2): the nine first-slot reads of a plane of cells are issued
//                      before the first is consumed, the walk past a foreign key is the rare case.  Then residual, Jacobian, the
//                      chunk's 29 subtree sums: a lane-xor butterfly (xor 1, 2, .. 32 = adjacent pairing), then the four waves
//   lz_solve_kernel    one wave per scan: a lane per sum finishes the tree over the chunks, lane 0 goes on alone; after stage A
//                      chooses the seed; solves (Cholesky, retraction) for the next pass's pose; after the final pass writes the five
//                      outputs
// The localisation has no atomics and reads no workspace word that an earlier kernel of the same call has not written.  No inline
// assembly, no scratch.
// What the localisation shares with register.hip -- the limits, the workspace, the seeds' half of the prep kernel, the correspondence
// kernel's source row and chunk sums, the tree over the chunks, the host's launch sequence -- and the Cholesky, its substitutions and
// the rotation of a quaternion are pose_common.h's (ps_*).
#include "map_common.h"
#include "pose_common.h"
#include "../../include/epcnet_localize.h"

#include <math.h>

#define LZ_THREADS 256
#define LZ_SUMS 29
#define LZ_MAX_M (1ll << 28)
#define LZ_HEAD 32             // int32 in front of the table (128 bytes)
#define LZ_ABSENT 0            //   [0] surfels not present   [1] out of range   [2] indexed   [3] duplicates
#define LZ_RANGE 1
#define LZ_INDEXED 2
#define LZ_DUP 3
#define LZ_HEAD_M 4            //   [4] M   [5], [6] the bits of voxel

// one slot of the table: 32 bytes, read as two 16-byte words
struct alignas(16) lz_slot {
    unsigned long long key;
    float c[3];
    float n[3];
};
static_assert(sizeof(lz_slot) == 32, "a slot is 32 bytes");

// the index: head | table (cap slots) | winner (cap int32)
struct lz_index {
    int32_t* head;
    lz_slot* table;
    int32_t* winner;
    unsigned long long mask;   // cap - 1
};
struct lz_index_layout_t { lz_index ix; size_t bytes; };
static lz_index_layout_t lz_index_layout(void* index, long long M) {
    epc_carver c(index);
    const unsigned long long cap = mp_cap(M);
    return {{c.take<int32_t>(LZ_HEAD, 128), c.take<lz_slot>(cap), c.take<int32_t>(cap, 16), cap - 1}, c.bytes()};
}

// ---- the index ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LZ_THREADS) void lz_clear_kernel(lz_index ix, long long M, double voxel) {
    const unsigned long long stride = (unsigned long long)gridDim.x * LZ_THREADS;
    const unsigned long long first = (unsigned long long)blockIdx.x * LZ_THREADS + threadIdx.x;
    const unsigned long long cap = ix.mask + 1;
    unsigned long long* const base = reinterpret_cast<unsigned long long*>(ix.table);
    for (unsigned long long i = first; i < cap * 4; i += stride) base[i] = (i & 3) == 0 ? MP_EMPTY : 0ull;
    for (unsigned long long i = first; i < cap; i += stride) ix.winner[i] = MP_NO_LEADER;
    if (first < LZ_HEAD) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(voxel);
        ix.head[first] = first == LZ_HEAD_M ? (int32_t)M : first == LZ_HEAD_M + 1 ? (int32_t)(bits & 0xffffffffull)
                                                         : first == LZ_HEAD_M + 2 ? (int32_t)(bits >> 32) : 0;
    }
}

// the cell of three float32 words under `voxel`: false unless every k_a lies in [-EPC_MAP_MAX_CELL, EPC_MAP_MAX_CELL)
__device__ __forceinline__ bool lz_cell(float x, float y, float z, double voxel, long long* k) {
#pragma clang fp contract(off)
    const double f0 = __builtin_floor((double)x / voxel), f1 = __builtin_floor((double)y / voxel), f2 = __builtin_floor((double)z / voxel);
    const double lim = (double)EPC_MAP_MAX_CELL;
    if (!(f0 >= -lim && f0 < lim && f1 >= -lim && f1 < lim && f2 >= -lim && f2 < lim)) return false;
    k[0] = (long long)f0, k[1] = (long long)f1, k[2] = (long long)f2;
    return true;
}

// surfel j: 0 present and in range (then k holds its cell), 1 not present, 2 out of range
__device__ __forceinline__ int lz_surfel_kind(const float* __restrict__ anchor, const float* __restrict__ centroid,
                                              const float* __restrict__ normal, long long j, double voxel, long long* k) {
    const float a0 = anchor[3 * j], a1 = anchor[3 * j + 1], a2 = anchor[3 * j + 2];
    if (!(epc_finite3(a0, a1, a2) && epc_finite3(centroid[3 * j], centroid[3 * j + 1], centroid[3 * j + 2]) &&
          epc_finite3(normal[3 * j], normal[3 * j + 1], normal[3 * j + 2])))
        return 1;
    return lz_cell(a0, a1, a2, voxel, k) ? 0 : 2;
}

__global__ __launch_bounds__(LZ_THREADS) void lz_insert_kernel(const float* __restrict__ anchor, const float* __restrict__ centroid,
                                                               const float* __restrict__ normal, long long M, double voxel, lz_index ix) {
    const long long j = (long long)blockIdx.x * LZ_THREADS + threadIdx.x;
    if (j >= M) return;
    long long k[3];
    if (lz_surfel_kind(anchor, centroid, normal, j, voxel, k)) return;
    const unsigned long long key = mp_key(k[0], k[1], k[2]);
    unsigned long long s = mp_hash(key) & ix.mask;
    // (at most M keys in >= 2 M + 1 slots: an empty slot always exists; the bound only ends a walk that cannot happen)
    for (unsigned long long probes = 0; probes <= ix.mask; ++probes) {
        unsigned long long* kp = &ix.table[s].key;
        unsigned long long have = __atomic_load_n(kp, __ATOMIC_RELAXED);
        if (have == MP_EMPTY) {
            have = atomicCAS(kp, MP_EMPTY, key);
            if (have == MP_EMPTY) have = key;
        }
        if (have == key) {
            int32_t* w = &ix.winner[s];
            if (mp_load(w) > (int)j) atomicMin(w, (int)j);      // (it only falls: a stale read costs an atomic)
            return;
        }
        s = (s + 1) & ix.mask;
    }
}

// the slot of `key`, or -1: the walk ends at the key or at an empty slot
__device__ __forceinline__ long long lz_find(const lz_index& ix, unsigned long long key) {
    unsigned long long s = mp_hash(key) & ix.mask;
    for (unsigned long long probes = 0; probes <= ix.mask; ++probes) {
        const unsigned long long have = ix.table[s].key;
        if (have == key) return (long long)s;
        if (have == MP_EMPTY) return -1;
        s = (s + 1) & ix.mask;
    }
    return -1;
}

__global__ __launch_bounds__(LZ_THREADS) void lz_fill_kernel(const float* __restrict__ anchor, const float* __restrict__ centroid,
                                                             const float* __restrict__ normal, long long M, double voxel, lz_index ix) {
    __shared__ int kinds[4];
    const int tid = threadIdx.x;
    if (tid < 4) kinds[tid] = 0;
    __syncthreads();
    const long long j = (long long)blockIdx.x * LZ_THREADS + tid;
    if (j < M) {
        long long k[3];
        const int kind = lz_surfel_kind(anchor, centroid, normal, j, voxel, k);
        int what = kind == 1 ? LZ_ABSENT : LZ_RANGE;
        if (kind == 0) {
            const long long s = lz_find(ix, mp_key(k[0], k[1], k[2]));
            what = LZ_DUP;
            if (s >= 0 && ix.winner[s] == (int)j) {
                what = LZ_INDEXED;
                lz_slot* t = ix.table + s;
#pragma unroll
                for (int a = 0; a < 3; ++a) t->c[a] = centroid[3 * j + a], t->n[a] = normal[3 * j + a];
            }
        }
        atomicAdd(&kinds[what], 1);
    }
    __syncthreads();
    if (tid < 4 && kinds[tid]) atomicAdd(&ix.head[tid], kinds[tid]);
}

__global__ void lz_num_kernel(lz_index ix, int32_t* __restrict__ num) {
    if (threadIdx.x == 0) {
        num[0] = ix.head[LZ_INDEXED];
        num[1] = ix.head[LZ_ABSENT];
        num[2] = ix.head[LZ_DUP];
        num[3] = ix.head[LZ_RANGE];
    }
}

static bool lz_voxel_ok(double voxel) { return __builtin_isfinite(voxel) && voxel >= 1.0 / 1048576.0 && voxel <= 1048576.0; }

extern "C" size_t epcnet_surfel_index_bytes(long long M) {
    return M >= 1 && M <= LZ_MAX_M ? lz_index_layout(nullptr, M).bytes : 0;
}

extern "C" int epcnet_surfel_index(const float* anchor, const float* centroid, const float* normal, long long M, const double* params,
                                   void* index, size_t index_bytes, int32_t* num, void* stream) {
    EPC_CHECK_ARG(anchor && centroid && normal && params && index && num, "null pointer");
    EPC_CHECK_ARG(M >= 1 && M <= LZ_MAX_M, "need 1 <= M <= 2^28");
    const double voxel = params[0];
    EPC_CHECK_ARG(lz_voxel_ok(voxel), "voxel must be finite and in [2^-20, 2^20]");
    for (int i = 1; i < EPC_LOCALIZE_INDEX_PARAMS; ++i) EPC_CHECK_ARG(params[i] == 0.0, "the three reserved parameters must be 0");
    EPC_CHECK_ARG(epc_aligned16(index), "index must be 16-byte aligned");
    EPC_CHECK_WORKSPACE_BYTES(index_bytes, epcnet_surfel_index_bytes(M));
    const lz_index ix = lz_index_layout(index, M).ix;
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long clear_blocks = ((ix.mask + 1) * 4 + LZ_THREADS - 1) / LZ_THREADS;
    hipLaunchKernelGGL(lz_clear_kernel, dim3((unsigned)(clear_blocks < 65536 ? clear_blocks : 65536)), dim3(LZ_THREADS), 0, st, ix, M, voxel);
    EPC_CHECK_LAUNCH();
    const unsigned blocks = (unsigned)((M + LZ_THREADS - 1) / LZ_THREADS);
    hipLaunchKernelGGL(lz_insert_kernel, dim3(blocks), dim3(LZ_THREADS), 0, st, anchor, centroid, normal, M, voxel, ix);
    EPC_CHECK_LAUNCH();
    hipLaunchKernelGGL(lz_fill_kernel, dim3(blocks), dim3(LZ_THREADS), 0, st, anchor, centroid, normal, M, voxel, ix);
    EPC_CHECK_LAUNCH();
    hipLaunchKernelGGL(lz_num_kernel, dim3(1), dim3(64), 0, st, ix, num);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}

// ---- launch 1 of the localisation: the scans ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LZ_THREADS) void lz_prep_kernel(const float* __restrict__ scans, int n, const double* __restrict__ seeds,
                                                             int num_seeds, const int32_t* __restrict__ head, long long M, double voxel,
                                                             int32_t* __restrict__ state, int32_t* __restrict__ run_a,
                                                             double* __restrict__ cur) {
    const int q = blockIdx.x, tid = threadIdx.x;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(voxel);
    const bool index_ok = head[LZ_HEAD_M] == (int32_t)M && head[LZ_HEAD_M + 1] == (int32_t)(bits & 0xffffffffull) &&
                          head[LZ_HEAD_M + 2] == (int32_t)(bits >> 32);                       // (uniform)
    const float* __restrict__ src = scans + (size_t)q * n * 3;
    int rows[1] = {0};
    for (int i = tid; i < n; i += LZ_THREADS) rows[0] += epc_finite3(src[3 * i], src[3 * i + 1], src[3 * i + 2]) ? 1 : 0;
    ps_prep_item(q, index_ok, rows, seeds, num_seeds, state, run_a, cur);
}

// ---- the correspondence pass -------------------------------------------------------------------------------------------------------------
// r_c of the definition: float64, every operation rounded once
__device__ __forceinline__ double lz_rotate_row(const double* __restrict__ m, double x, double y, double z) {
#pragma clang fp contract(off)
    return (m[0] * x + m[1] * y) + m[2] * z;
}
__device__ __forceinline__ float lz_place(double r, double t) {
#pragma clang fp contract(off)
    return (float)(r + t);
}
// d2 of the definition
__device__ __forceinline__ float lz_d2(float px, float py, float pz, float cx, float cy, float cz) {
#pragma clang fp contract(off)
    const float dx = px - cx, dy = py - cy, dz = pz - cz;
    return (dx * dx + dy * dy) + dz * dz;
}

// One cell's candidate against the running minimum: (a, b) is the cell's first slot `s`, already read.  A foreign key in front is the
// rare case (linear probing; an empty slot always exists, the bound ends a walk on a table that is not an index).  key == MP_EMPTY:
// the cell does not count.
__device__ __forceinline__ void lz_candidate(const uint4* __restrict__ words, unsigned long long mask, unsigned long long key,
                                             unsigned long long s, uint4 a, uint4 b, float p0, float p1, float p2, float& best, float& c0,
                                             float& c1, float& c2, float& n0, float& n1, float& n2) {
    if (key == MP_EMPTY) return;
    unsigned long long have = ((unsigned long long)a.y << 32) | a.x;
    for (unsigned long long probes = 0; have != key && have != MP_EMPTY && probes < mask; ++probes) {
        s = (s + 1) & mask;
        a = words[2 * s], b = words[2 * s + 1];
        have = ((unsigned long long)a.y << 32) | a.x;
    }
    if (have != key) return;
    const float cx = __uint_as_float(a.z), cy = __uint_as_float(a.w), cz = __uint_as_float(b.x);
    const float d2 = lz_d2(p0, p1, p2, cx, cy, cz);
    if (d2 < best) {                                   // (a NaN never wins; a tie keeps the earlier candidate)
        best = d2;
        c0 = cx, c1 = cy, c2 = cz;
        n0 = __uint_as_float(b.y), n1 = __uint_as_float(b.z), n2 = __uint_as_float(b.w);
    }
}

// poses (Q, num_seeds, 12); run (Q, num_seeds): 0 = this pass is not wanted, nothing is written; sums (Q, num_seeds, chunks, 29).
// Grid (Q, num_seeds, chunks).  (A run flag is only set where the index records this M: mask is the table's.)
__global__ __launch_bounds__(PS_CHUNK) void lz_corr_kernel(const float* __restrict__ scans, int n, const double* __restrict__ poses,
                                                           const int32_t* __restrict__ run, const lz_slot* __restrict__ table,
                                                           unsigned long long mask, double voxel, float gate2,
                                                           double* __restrict__ sums) {
    __shared__ double part[PS_CHUNK / 64][LZ_SUMS];
    const int q = blockIdx.x, h = blockIdx.y, chunk = blockIdx.z, tid = threadIdx.x;
    const size_t qh = (size_t)q * gridDim.y + h;
    if (!run[qh]) return;
    float sx, sy, sz;
    bool present;
    ps_corr_row(scans + (size_t)q * n * 3, n, chunk, sx, sy, sz, present);
    const double* __restrict__ m = poses + qh * 12;
    const double r0 = lz_rotate_row(m, sx, sy, sz), r1 = lz_rotate_row(m + 4, sx, sy, sz), r2 = lz_rotate_row(m + 8, sx, sy, sz);
    const float p0 = lz_place(r0, m[3]), p1 = lz_place(r1, m[7]), p2 = lz_place(r2, m[11]);
    float best = INFINITY, c0 = 0.f, c1 = 0.f, c2 = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
    if (chunk * PS_CHUNK + (tid & ~63) < n) {          // wave-uniform: a wave wholly behind the scan has nothing to look up
        long long k[3] = {0, 0, 0};
        bool any = false;
        if (present) {
#pragma clang fp contract(off)
            const double f0 = __builtin_floor((double)p0 / voxel), f1 = __builtin_floor((double)p1 / voxel),
                         f2 = __builtin_floor((double)p2 / voxel);
            const double lim = (double)EPC_MAP_MAX_CELL;
            // (a cell k + o can only count when k_a lies in [-lim - 1, lim]; false for a NaN)
            any = f0 >= -lim - 1.0 && f0 <= lim && f1 >= -lim - 1.0 && f1 <= lim && f2 >= -lim - 1.0 && f2 <= lim;
            if (any) k[0] = (long long)f0, k[1] = (long long)f1, k[2] = (long long)f2;
        }
        const uint4* __restrict__ words = reinterpret_cast<const uint4*>(table);
#pragma unroll 1
        for (int o2 = -1; o2 <= 1; ++o2) {
            const long long g2 = k[2] + o2;
            const bool in2 = any && g2 >= -EPC_MAP_MAX_CELL && g2 < EPC_MAP_MAX_CELL;
            unsigned long long key[9], at[9];
            uint4 lo[9], hi[9];
            // the plane's nine first-slot reads, issued before the first is consumed (a cell that does not count reads slot 0 under
            // the key of no cell)
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                const long long g1 = k[1] + (e / 3 - 1), g0 = k[0] + (e % 3 - 1);
                const bool in = in2 && g1 >= -EPC_MAP_MAX_CELL && g1 < EPC_MAP_MAX_CELL && g0 >= -EPC_MAP_MAX_CELL && g0 < EPC_MAP_MAX_CELL;
                key[e] = in ? mp_key(g0, g1, g2) : MP_EMPTY;
                at[e] = in ? mp_hash(key[e]) & mask : 0ull;
                lo[e] = words[2 * at[e]], hi[e] = words[2 * at[e] + 1];
            }
#pragma unroll
            for (int e = 0; e < 9; ++e) lz_candidate(words, mask, key[e], at[e], lo[e], hi[e], p0, p1, p2, best, c0, c1, c2, n0, n1, n2);
        }
    }
    const bool acc = best <= gate2;                    // gate2 is finite: a lane that found nothing (+Inf) fails
    double v[LZ_SUMS];
    {
#pragma clang fp contract(off)
        const double a = acc ? 1.0 : 0.0;
        const double N0 = acc ? (double)n0 : 0.0, N1 = acc ? (double)n1 : 0.0, N2 = acc ? (double)n2 : 0.0;
        const double R0 = acc ? r0 : 0.0, R1 = acc ? r1 : 0.0, R2 = acc ? r2 : 0.0;
        const double d0 = acc ? (double)p0 - (double)c0 : 0.0, d1 = acc ? (double)p1 - (double)c1 : 0.0,
                     d2 = acc ? (double)p2 - (double)c2 : 0.0;
        const double e = (N0 * d0 + N1 * d1) + N2 * d2;
        double J[6];
        J[0] = R1 * N2 - R2 * N1;
        J[1] = R2 * N0 - R0 * N2;
        J[2] = R0 * N1 - R1 * N0;
        J[3] = N0, J[4] = N1, J[5] = N2;
        v[0] = a;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = r; c < 6; ++c) v[1 + r * (13 - r) / 2 + (c - r)] = J[r] * J[c];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) v[22 + r] = J[r] * e;
        v[28] = e * e;
    }
    ps_chunk_sums(v, part, sums + (qh * gridDim.z + chunk) * LZ_SUMS);
}

// ---- the solve -----------------------------------------------------------------------------------------------------------------------------
// one Gauss-Newton step from the 29 sums on `pose`; false on a failed pivot or a non-finite word in the new pose
__device__ __forceinline__ bool lz_step(const double (&S)[LZ_SUMS], double (&pose)[12]) {
#pragma clang fp contract(off)
    double Lc[21], r[6], d[6], C[9];
    bool ok = ps_chol6(&S[1], Lc);                     // H's upper triangle by rows is sums 1 .. 21
#pragma unroll
    for (int i = 0; i < 6; ++i) r[i] = -S[22 + i];
    ps_chol6_solve(Lc, r, d);
    ps_rotation<3>(1.0, 0.5 * d[0], 0.5 * d[1], 0.5 * d[2], C);
    double next[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) next[4 * i + j] = ps_d3(C[3 * i], C[3 * i + 1], C[3 * i + 2], pose[j], pose[4 + j], pose[8 + j]);
        next[4 * i + 3] = pose[4 * i + 3] + d[3 + i];
    }
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        ok = ok && __builtin_isfinite(next[c]);
        pose[c] = next[c];
    }
    return ok;
}

// One wave per scan, behind a correspondence launch whose sums are (Q, pass_seeds, chunks, 29): lane s finishes sum s (and, after stage
// A, lane k the count and sums[28] of seed k); lane 0 goes on alone.
//   select: the pass was stage A (pass_seeds = H): choose the seed, copy it to cur (where seeds is not NULL)
//   solve:  the next pose from the sums into cur, and run_b for the next pass
//   output: the pass was the final one: write pose, fit, hessian, info and status
__global__ __launch_bounds__(64) void lz_solve_kernel(const double* __restrict__ sums, int pass_seeds, int chunks,
                                                      const double* __restrict__ seeds, const int32_t* __restrict__ run_a, int min_pairs,
                                                      int select, int solve, int output, int32_t* __restrict__ state,
                                                      int32_t* __restrict__ run_b, double* __restrict__ cur, double* __restrict__ pose_out,
                                                      double* __restrict__ fit_out, double* __restrict__ hessian_out,
                                                      int32_t* __restrict__ info_out, int32_t* __restrict__ status_out) {
    __shared__ double S_s[LZ_SUMS];
    __shared__ double count_s[PS_MAX_SEEDS], cost_s[PS_MAX_SEEDS];
    __shared__ int best_s;
    const int q = blockIdx.x, lane = threadIdx.x;
    int32_t* st = state + (size_t)q * PS_STATE;
    int status = st[0], best = st[1];                  // (uniform over the wave)
    const int rows = st[2];
    __syncthreads();                                   // (lane 0 writes st behind everybody's read)
    if (status == 0) {
        int h = 0;
        if (select) {
            const bool ran = lane < pass_seeds && run_a[(size_t)q * pass_seeds + lane] != 0;
            if (ran) {
                const double* cs = sums + ((size_t)q * pass_seeds + lane) * chunks * LZ_SUMS;
                count_s[lane] = ps_finish_sum<LZ_SUMS>(cs, chunks, 0), cost_s[lane] = ps_finish_sum<LZ_SUMS>(cs, chunks, 28);
            }
            __syncthreads();
            if (lane == 0) {
                double bc = 0.0, bd = 0.0;
                int b = -1;
                for (int k = 0; k < pass_seeds; ++k) {
                    if (!run_a[(size_t)q * pass_seeds + k]) continue;
                    const double c = count_s[k], d = cost_s[k];
                    if (b < 0 || c > bc || (c == bc && d < bd)) b = k, bc = c, bd = d;
                }
                best_s = b;                            // >= 0: status 0 says that a seed ran
            }
            __syncthreads();
            h = best = best_s;
        }
        if (lane < LZ_SUMS) S_s[lane] = ps_finish_sum<LZ_SUMS>(sums + ((size_t)q * pass_seeds + h) * chunks * LZ_SUMS, chunks, lane);
    }
    __syncthreads();
    if (lane != 0) return;
    double S[LZ_SUMS], pose[12];
    double* mine = cur + (size_t)q * 12;
    if (status == 0) {
        if (select) {
            st[1] = best;
            if (seeds) {
#pragma unroll
                for (int c = 0; c < 12; ++c) mine[c] = seeds[((size_t)q * pass_seeds + best) * 12 + c];
            }
        }
#pragma unroll
        for (int k = 0; k < LZ_SUMS; ++k) S[k] = S_s[k];
        if (S[0] < (double)min_pairs) {
            status = EPC_STATUS_NO_FIT;
        } else if (solve) {
#pragma unroll
            for (int c = 0; c < 12; ++c) pose[c] = mine[c];
            if (lz_step(S, pose)) {
#pragma unroll
                for (int c = 0; c < 12; ++c) mine[c] = pose[c];
            } else {
                status = EPC_STATUS_NO_FIT;
            }
        }
        if (status) st[0] = status;
    }
    if (solve) run_b[q] = status == 0 ? 1 : 0;
    if (!output) return;
    const double nan = epc_nan_f64();
#pragma unroll
    for (int c = 0; c < 12; ++c) pose_out[(size_t)q * 12 + c] = status == 0 ? mine[c] : nan;
    {
#pragma clang fp contract(off)
        fit_out[2 * (size_t)q] = status == 0 ? S[28] / S[0] : nan;
        fit_out[2 * (size_t)q + 1] = status == 0 ? S[0] / (double)rows : nan;
    }
#pragma unroll
    for (int c = 0; c < 21; ++c) hessian_out[(size_t)q * 21 + c] = status == 0 ? S[1 + c] : nan;
    info_out[4 * (size_t)q] = status == 0 ? best : -1;
    info_out[4 * (size_t)q + 1] = status == 0 ? (int)S[0] : 0;
    info_out[4 * (size_t)q + 2] = rows;
    info_out[4 * (size_t)q + 3] = 0;
    status_out[q] = status;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t epcnet_scan_localize_workspace_bytes(int Q, int H, int n) {
    return ps_shape_ok(Q, H, n) ? ps_layout<LZ_SUMS>(nullptr, Q, H, n).bytes : 0;
}

extern "C" int epcnet_scan_localize(const float* scans, int Q, int n, const double* seeds, int H, const void* index, size_t index_bytes,
                                    const float* centroid, const float* normal, long long M, const double* params, double* pose,
                                    double* fit, double* hessian, int32_t* info, int32_t* status, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    EPC_CHECK_ARG(scans && index && centroid && normal && params && pose && fit && hessian && info && status && workspace, "null pointer");
    EPC_CHECK_ARG(epc_aligned16(scans) && epc_aligned16(index), "scans and index must be 16-byte aligned");
    EPC_CHECK_ARG(ps_shape_ok(Q, H, n), "need n a multiple of 32 in [32, 4096], 0 <= Q <= 2^20, 1 <= H <= 64");
    EPC_CHECK_ARG(seeds || H == 1, "seeds is NULL: H must be 1 (the identity)");
    EPC_CHECK_ARG(M >= 1 && M <= LZ_MAX_M, "need 1 <= M <= 2^28");
    const double voxel = params[0], max_dist = params[1], iters = params[2], pairs = params[3];
    EPC_CHECK_ARG(lz_voxel_ok(voxel), "voxel must be finite and in [2^-20, 2^20]");
    EPC_CHECK_ARG(isfinite(max_dist) && max_dist > 0.0, "max_dist must be finite and > 0");
    EPC_CHECK_ARG(iters >= 0.0 && iters <= 64.0 && iters == __builtin_floor(iters), "iterations must be an integer value in [0, 64]");
    EPC_CHECK_ARG(pairs >= 6.0 && pairs <= (double)n && pairs == __builtin_floor(pairs), "min_pairs must be an integer value in [6, n]");
    for (int i = 4; i < EPC_LOCALIZE_PARAMS; ++i) EPC_CHECK_ARG(params[i] == 0.0, "the four reserved parameters must be 0");
    if (Q == 0) return EPC_OK;
    EPC_CHECK_WORKSPACE_BYTES(index_bytes, epcnet_surfel_index_bytes(M));
    EPC_CHECK_WORKSPACE(workspace, workspace_bytes, epcnet_scan_localize_workspace_bytes(Q, H, n));
    const int iterations = (int)iters, min_pairs = (int)pairs;
    const float gate2 = ps_gate2(max_dist);
    const int chunks = ps_chunks(n);
    const lz_index ix = lz_index_layout(const_cast<void*>(index), M).ix;
    const ps_ws w = ps_layout<LZ_SUMS>(workspace, Q, H, n);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lz_prep_kernel, dim3(Q), dim3(LZ_THREADS), 0, st, scans, n, seeds, H, ix.head, M, voxel, w.state, w.run_a, w.cur);
    return ps_drive(
        __func__, seeds, H, iterations, w,
        [&](int seed_count, const double* poses, const int32_t* run) {
            hipLaunchKernelGGL(lz_corr_kernel, dim3(Q, seed_count, chunks), dim3(PS_CHUNK), 0, st, scans, n, poses, run, ix.table, ix.mask, voxel,
                               gate2, w.sums);
        },
        [&](int pass_seeds, int select, int solve, int output) {
            hipLaunchKernelGGL(lz_solve_kernel, dim3(Q), dim3(64), 0, st, w.sums, pass_seeds, chunks, seeds, w.run_a, min_pairs, select, solve,
                               output, w.state, w.run_b, w.cur, pose, fit, hessian, info, status);
        });
}
