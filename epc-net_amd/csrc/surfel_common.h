// ONE definition of what the two surfel files share (surfel.hip: epcnet_map_surfels, the map built in one call; growmap.hip:
// epcnet_surfel_map_add, the map that grows across calls) and that follows the 128-byte slot: the slot and its cleared state, the
// parameters and their refusals, a tile's rows -> kinds and lattice positions, a row's position and its claim to lead on the way into
// a slot, the sixteen-lane adds, the Jacobi rotation and the pool-and-solve.  What does not depend on the slot's layout -- key and
// cell, the claim loop, the lookup, the leaders' scan -- is map_common.h's, shared with map.hip.  The bit contract of
// include/epcnet_surfels.h forbids a second copy of the float64 sequence: both files' outputs come out of sf_pool_solve.  Device
// helpers are __forceinline__: a kernel's code is what it was with the piece written out.
#ifndef EPC_SURFEL_COMMON_H
#define EPC_SURFEL_COMMON_H
#include "map_common.h"
#include "../../include/epcnet_surfels.h"

// one slot of the table: sixteen 64-bit words, 128 bytes.  surfel.hip uses `leader` of the last two words; growmap.hip all four: the
// voxel's number + 1 (0: not numbered yet) and the epochs (calls) in which the slot last received a row and was last marked dirty
struct sf_slot {
    unsigned long long key;
    unsigned long long cnt;
    unsigned long long sum[3];     // of w_a & 4095: the mean of map_points
    unsigned long long A[3];       // of u_a = (w_a & 4095) >> 4
    unsigned long long B[6];       // of u_a u_b: 00 01 02 11 12 22
    int32_t leader;
    int32_t number;
    uint32_t touched;
    uint32_t dirty;
};
static_assert(sizeof(sf_slot) == 128, "a slot is sixteen 64-bit words");

// word e of a cleared slot: the empty key, no leader (word 14: leader in the low half, number 0), zero sums and epochs
__device__ __forceinline__ unsigned long long sf_cleared_word(unsigned e) {
    return e == 0 ? MP_EMPTY : e == 14 ? (unsigned long long)MP_NO_LEADER : 0ull;
}
// every slot of the table cleared by the threads first, first + stride, ...: sixteen lanes per slot, one word each -- a wave-instruction
// stores four whole slots
__device__ __forceinline__ void sf_clear_table(sf_slot* table, unsigned long long mask, unsigned long long first, unsigned long long stride) {
    const unsigned long long words = (mask + 1) * 16;
    unsigned long long* const base = reinterpret_cast<unsigned long long*>(table);
    for (unsigned long long i = first; i < words; i += stride) base[i] = sf_cleared_word((unsigned)(i & 15));
}
// the workgroups of MP_THREADS that a clearing launch takes: a thread per word, at most 65536 of them
static inline unsigned sf_clear_blocks(unsigned long long mask) {
    const unsigned long long blocks = ((mask + 1) * 16 + MP_THREADS - 1) / MP_THREADS;
    return (unsigned)(blocks < 65536 ? blocks : 65536);
}

struct sf_params {
    double voxel, step, step8;     // step = fl(voxel / 4096), step8 = fl(voxel / 256)
    long long min_count, min_support;
    int ring;
};

// ---- host: the rules of the eight doubles (those of the three counts: mp_shape_refusal) ---------------------------------------------------
// why `params` (EPC_SURFEL_PARAMS doubles in host memory) are refused, or NULL
static inline const char* sf_params_refusal(const double* params) {
    const double voxel = params[0], min_count = params[1], ring = params[2], min_support = params[3];
    if (!(__builtin_isfinite(voxel) && voxel >= 1.0 / 1048576.0 && voxel <= 1048576.0)) return "voxel must be finite and in [2^-20, 2^20]";
    if (!(min_count >= 1.0 && min_count < 2147483648.0 && min_count == __builtin_floor(min_count)))
        return "min_count must be an integer value in [1, 2^31)";
    if (!(ring >= 0.0 && ring <= (double)EPC_SURFEL_MAX_RING && ring == __builtin_floor(ring)))
        return "ring must be an integer value in [0, EPC_SURFEL_MAX_RING]";
    if (!(min_support >= 3.0 && min_support < 2147483648.0 && min_support == __builtin_floor(min_support)))
        return "min_support must be an integer value in [3, 2^31)";
    for (int i = 4; i < EPC_SURFEL_PARAMS; ++i)
        if (!(params[i] == 0.0)) return "the four reserved parameters must be 0";
    return nullptr;
}
static inline sf_params sf_params_of(const double* params) {
    sf_params pr;
    pr.voxel = params[0];
    pr.step = params[0] / 4096.0;
    pr.step8 = params[0] / 256.0;
    pr.min_count = (long long)params[1];
    pr.min_support = (long long)params[3];
    pr.ring = (int)params[2];
    return pr;
}

// ---- the rows of a tile -----------------------------------------------------------------------------------------------------------------
// what an insert kernel keeps in LDS
struct sf_tile_lds {
    double pose[12];
    int c_first, c_last;
    int kinds[3];
    int slot[MP_TILE];                     // the slot of every row of the tile, negative: nothing to add
    unsigned short pos[MP_TILE][4];        // its w_a & 4095
};

// Row r = r0 + tid of the tile that begins at r0: 0 kept (then w holds the lattice coordinates), 1 absent, 2 out of range, 4 no row of any
// cloud; a kind below 4 is counted in lds.kinds.  Every thread of the workgroup calls it (two barriers).
__device__ __forceinline__ int sf_tile_row(const float* __restrict__ points, const int32_t* __restrict__ offsets, long long num_rows,
                                           int num_clouds, const double* __restrict__ poses, const double* __restrict__ origin,
                                           double voxel, sf_tile_lds& lds, long long r0, long long* w) {
    const int tid = threadIdx.x;
    const long long r = r0 + tid;
    const long long r1 = r0 + MP_TILE < num_rows ? r0 + MP_TILE : num_rows;                  // the tile's end
    if (tid == 0) lds.c_first = first_scan_behind(offsets, 0, num_clouds, r0);               // num_clouds: behind every cloud
    if (tid == 1) lds.c_last = first_scan_behind(offsets, 0, num_clouds, r1 - 1);
    if (tid < 3) lds.kinds[tid] = 0;
    __syncthreads();
    const int cf = lds.c_first, cl = lds.c_last;
    if (tid < 12 && cf < num_clouds) lds.pose[tid] = poses[(size_t)cf * 12 + tid];
    __syncthreads();
    if (r >= num_rows) return 4;
    const int c = cf == cl ? cf : first_scan_behind(offsets, cf, cl, r);
    if (!(c < num_clouds && r >= (long long)offsets[c])) return 4;
    double m[12], d[3];
    if (c == cf) {
#pragma unroll
        for (int e = 0; e < 12; ++e) m[e] = lds.pose[e];
    } else {
#pragma unroll
        for (int e = 0; e < 12; ++e) m[e] = poses[(size_t)c * 12 + e];
    }
    {
#pragma clang fp contract(off)
        d[0] = m[3] - origin[0], d[1] = m[7] - origin[1], d[2] = m[11] - origin[2];
    }
    const int kind = mp_row(m, d, voxel, points[(size_t)r * 3], points[(size_t)r * 3 + 1], points[(size_t)r * 3 + 2], w);
    atomicAdd(&lds.kinds[kind], 1);
    return kind;
}

// on the way into a slot: the row's position in its cell, for the tile's adds
__device__ __forceinline__ void sf_stage_pos(sf_tile_lds& lds, int tid, const long long* w) {
    lds.pos[tid][0] = (unsigned short)(w[0] & 4095), lds.pos[tid][1] = (unsigned short)(w[1] & 4095);
    lds.pos[tid][2] = (unsigned short)(w[2] & 4095);
}
// and row r's claim to lead slot t (the leader only falls: a stale read costs an atomic)
__device__ __forceinline__ void sf_lead(sf_slot* t, long long r) {
    int32_t* lead = &t->leader;
    if (mp_load(lead) > (int)r) atomicMin(lead, (int)r);
}

// The tile's adds, behind a barrier that follows the last write of lds.slot / lds.pos: sixteen lanes per row, one per word of its slot
// (1 the count, 2..4 the 12-bit sums, 5..7 A, 8..13 B; the key's lane and the last two idle): a wave-instruction adds to four slots of 104
// contiguous bytes each.  NEGATE: the rows are taken OUT (growmap.hip's move) -- the two's-complement negation is added, unsigned wrap-around.
template <bool NEGATE = false>
__device__ __forceinline__ void sf_add_rows(sf_slot* __restrict__ table, const sf_tile_lds& lds) {
    const int tid = threadIdx.x, word = tid & 15;
    for (int it = 0; it < MP_TILE / 16; ++it) {
        const int row = it * 16 + (tid >> 4);
        const int sl = lds.slot[row];
        if (sl >= 0 && word >= 1 && word <= 13) {
            const unsigned long long p0 = lds.pos[row][0], p1 = lds.pos[row][1], p2 = lds.pos[row][2];
            const unsigned long long u0 = p0 >> 4, u1 = p1 >> 4, u2 = p2 >> 4;
            const unsigned long long x = word < 8 ? (word == 1 || word == 2 || word == 5 ? (word == 1 ? 1ull : word == 2 ? p0 : u0)
                                                                                         : (word == 3 ? p1 : word == 4 ? p2 : word == 6 ? u1 : u2))
                                                  : (word < 11 ? u0 : word < 13 ? u1 : u2);
            const unsigned long long y = word < 8 ? 1ull : (word == 8 ? u0 : word == 9 || word == 11 ? u1 : u2);
            atomicAdd(reinterpret_cast<unsigned long long*>(table + sl) + word, NEGATE ? 0ull - x * y : x * y);
        }
    }
}

// ---- a voxel's outputs ------------------------------------------------------------------------------------------------------------------
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

// map_points and count of voxel j from its slot (a voxel that a move emptied: count 0, NaN, nothing divided by)
__device__ __forceinline__ void sf_write_mean(const sf_slot* __restrict__ t, const sf_params& pr, long long j, float* __restrict__ map_points,
                                              int32_t* __restrict__ count) {
#pragma clang fp contract(off)
    const float nan = epc_nan_f32();
    const long long cnt = (long long)t->cnt;
    long long g0, g1, g2;
    mp_cell(t->key, g0, g1, g2);
    const unsigned long long by = cnt != 0 ? (unsigned long long)cnt : 1ull;
    const long long m0 = (long long)(t->sum[0] / by), m1 = (long long)(t->sum[1] / by), m2 = (long long)(t->sum[2] / by);
    const bool keep = cnt >= pr.min_count;
    map_points[(size_t)j * 3] = keep ? (float)((double)(g0 * 4096 + m0) * pr.step) : nan;
    map_points[(size_t)j * 3 + 1] = keep ? (float)((double)(g1 * 4096 + m1) * pr.step) : nan;
    map_points[(size_t)j * 3 + 2] = keep ? (float)((double)(g2 * 4096 + m2) * pr.step) : nan;
    count[j] = (int32_t)cnt;
}

// The surfel of the voxel in slot t: the (2 ring + 1)^3 cells around it are looked up (read-only), their moments pooled in int64, and
// the covariance, the Jacobi, the order and the normal run in float64 registers -> out[0..2] centroid, out[3..5] normal, out[6..8] eigen
// (0x7fc00000 for a surfel that is not valid); returns support.
__device__ __forceinline__ int32_t sf_pool_solve(const sf_slot* __restrict__ table, unsigned long long mask, const sf_slot* __restrict__ t,
                                                 const sf_params& pr, float* out) {
    const float nan = epc_nan_f32();
    const long long cnt = (long long)t->cnt;
    long long g0, g1, g2;
    mp_cell(t->key, g0, g1, g2);
    // the pool, in the frame of cell g: int64
    long long N = 0, S1x = 0, S1y = 0, S1z = 0, Sxx = 0, Sxy = 0, Sxz = 0, Syy = 0, Syz = 0, Szz = 0;
    const int ring = pr.ring;
    for (int o2 = -ring; o2 <= ring; ++o2) {
        const long long c2 = g2 + o2;
        if (!mp_in_range(c2)) continue;
        for (int o1 = -ring; o1 <= ring; ++o1) {
            const long long c1 = g1 + o1;
            if (!mp_in_range(c1)) continue;
            for (int o0 = -ring; o0 <= ring; ++o0) {
                const long long c0 = g0 + o0;
                if (!mp_in_range(c0)) continue;
                const long long at = mp_find(table, mask, mp_key(c0, c1, c2));
                if (at < 0) continue;
                const sf_slot* q = table + at;
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
    out[0] = oc0, out[1] = oc1, out[2] = oc2, out[3] = on0, out[4] = on1, out[5] = on2, out[6] = oe0, out[7] = oe1, out[8] = oe2;
    return (int32_t)N;
}

// voxel j's nine words and support from its slot
__device__ __forceinline__ void sf_write_surfel(const sf_slot* __restrict__ table, unsigned long long mask, const sf_slot* __restrict__ t,
                                                const sf_params& pr, long long j, float* __restrict__ centroid, float* __restrict__ normal,
                                                float* __restrict__ eigen, int32_t* __restrict__ support) {
    float out[9];
    support[j] = sf_pool_solve(table, mask, t, pr, out);
#pragma unroll
    for (int a = 0; a < 3; ++a) centroid[(size_t)j * 3 + a] = out[a], normal[(size_t)j * 3 + a] = out[3 + a], eigen[(size_t)j * 3 + a] = out[6 + a];
}

// NaN / 0 in the six output arrays' row j
__device__ __forceinline__ void sf_write_none(long long j, float* __restrict__ map_points, int32_t* __restrict__ count, float* __restrict__ centroid,
                                              float* __restrict__ normal, float* __restrict__ eigen, int32_t* __restrict__ support) {
    const float nan = epc_nan_f32();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        map_points[(size_t)j * 3 + a] = nan, centroid[(size_t)j * 3 + a] = nan;
        normal[(size_t)j * 3 + a] = nan, eigen[(size_t)j * 3 + a] = nan;
    }
    count[j] = 0, support[j] = 0;
}
#endif
