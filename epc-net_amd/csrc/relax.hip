// Trajectory relaxation (include/epcnet_trajectory.h; numpy restatement in tests/relax_ref.py): Gauss-Newton on a chain of T submap poses
// with L loop edges, in chain-increment variables, by preconditioned CG.  Every float64 operation is rounded once (contract off), the
// scans run in ONE order (eight Kogge-Stone steps over blocks of 256 nodes, the block totals scanned the same way), the sums in ONE order
// (adjacent pairing), so the result is the same bits on every run and equal to numpy's.
//
// poses, pairs, rel and weights are device data: every grid is sized from T and L alone, nothing is read back; what depends on the data
// (T_eff, which loops are used, whether anything is solved, a failed pivot, a CG solve that ended early) is a flag in the workspace
// that the kernels behind it read.
//   prep      rx_teff_kernel (one workgroup), rx_loops_kernel (a thread per loop: the skip rules), rx_count_kernel and rx_fill_kernel (a
//             thread per node: count, scan, stable fill of the node's list of loops, ascending; the state R, c and the chain's Z)
//   linearise rx_lin_chain_kernel (J, J^T W r, D = J^T W J and its Cholesky factor per chain edge), rx_lin_loops_kernel, rx_cost_kernel
//   H p       rx_scan_kernel (block scan of p), rx_eta_kernel (+ the blocks before), rx_loop_apply_kernel (u_e per loop),
//             rx_gather_kernel (g from the node's list, block scan), rx_product_kernel (v_n + scan(g), the partial of p . Hp)
//   CG        rx_update_kernel (alpha, x, r, z = D^-1 r, the partial of r . z), rx_direction_kernel (beta, p); rx_start_kernel opens a solve
//   step      rx_scan_kernel on x, rx_retract_kernel
//   rx_finish_kernel writes poses_out, and everything where nothing was solved
// No atomics, no flag one workgroup waits on, no grid barrier, no word read that an earlier kernel of the same call has not written.
// The three-term dot, the 6 x 6 Cholesky, its substitutions and the rotation of a quaternion are pose_common.h's (ps_*), shared with
// localize.hip and register.hip.
#include "pose_common.h"
#include "../../include/epcnet_trajectory.h"

#include <math.h>

#define RX_BLOCK 256
#define RX_MAX_T 65536
#define RX_MAX_L (1 << 20)
#define RX_MAX_BLOCKS (RX_MAX_T / RX_BLOCK)          // 256: the block totals fit one more block scan
#define RX_MAX_LBLOCKS (RX_MAX_L / RX_BLOCK)         // 4096 partials of the loops' cost: 16 per thread of the finishing workgroup
enum { RX_TE = 0, RX_ACTIVE = 1, RX_FAIL = 2, RX_USED = 3, RX_FLAGS = 4 };

// element k of item i of a structure-of-arrays buffer of `stride` items
#define RX_AT(buf, k, i, stride) (buf)[(size_t)(k) * (size_t)(stride) + (size_t)(i)]

static inline int rx_blocks(int n) { return (n + RX_BLOCK - 1) / RX_BLOCK; }

// ---- the arithmetic of the definition ------------------------------------------------------------------------------------------------------
// An edge (a, b, Z, w_t, w_r) at the state (Ra, ca), (Rb, cb); R row-major 3 x 3, Z row-major [Z_R | z_t] 3 x 4.
// J = [[A, B], [0, C]] as J[0..9) = A, J[9..18) = B, J[18..27) = C row-major; b = J^T W r; returns the edge's cost.
__device__ __forceinline__ double rx_linearise(const double (&Ra)[9], const double (&Rb)[9], const double (&ca)[3], const double (&cb)[3],
                                               const double (&Z)[12], double wt, double wr, double (&J)[27], double (&b)[6]) {
#pragma clang fp contract(off)
    double dc[3], rt[3], rR[3], M[9], E[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) dc[i] = cb[i] - ca[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) rt[i] = ps_d3(Ra[i], Ra[3 + i], Ra[6 + i], dc[0], dc[1], dc[2]) - Z[4 * i + 3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) M[3 * i + j] = ps_d3(Ra[i], Ra[3 + i], Ra[6 + i], Rb[j], Rb[3 + j], Rb[6 + j]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) E[3 * i + j] = ps_d3(Z[i], Z[4 + i], Z[8 + i], M[j], M[3 + j], M[6 + j]);
    }
    rR[0] = 0.5 * (E[7] - E[5]);
    rR[1] = 0.5 * (E[2] - E[6]);
    rR[2] = 0.5 * (E[3] - E[1]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) J[3 * i + j] = Ra[3 * j + i];                     // A = Ra^T
    }
    const double x = cb[0], y = cb[1], z = cb[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                                     // B = -A [cb]x
        J[9 + 3 * i] = J[3 * i + 2] * y - J[3 * i + 1] * z;
        J[9 + 3 * i + 1] = J[3 * i] * z - J[3 * i + 2] * x;
        J[9 + 3 * i + 2] = J[3 * i + 1] * x - J[3 * i] * y;
    }
    const double tr = (E[0] + E[4]) + E[8];
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) G[3 * i + j] = i == j ? tr - E[4 * i] : -E[3 * j + i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                                     // C = 1/2 G Rb^T
#pragma unroll
        for (int j = 0; j < 3; ++j) J[18 + 3 * i + j] = 0.5 * ps_d3(G[3 * i], G[3 * i + 1], G[3 * i + 2], Rb[3 * j], Rb[3 * j + 1], Rb[3 * j + 2]);
    }
    const double t0 = wt * rt[0], t1 = wt * rt[1], t2 = wt * rt[2];
    const double r0 = wr * rR[0], r1 = wr * rR[1], r2 = wr * rR[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        b[j] = ps_d3(J[j], J[3 + j], J[6 + j], t0, t1, t2);
        b[3 + j] = ps_d3(J[9 + j], J[12 + j], J[15 + j], t0, t1, t2) + ps_d3(J[18 + j], J[21 + j], J[24 + j], r0, r1, r2);
    }
    return wt * ((rt[0] * rt[0] + rt[1] * rt[1]) + rt[2] * rt[2]) + wr * ((rR[0] * rR[0] + rR[1] * rR[1]) + rR[2] * rR[2]);
}

// u = J^T W J d
__device__ __forceinline__ void rx_apply(const double (&J)[27], double wt, double wr, const double (&d)[6], double (&u)[6]) {
#pragma clang fp contract(off)
    double yt[3], yr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        yt[i] = wt * (ps_d3(J[3 * i], J[3 * i + 1], J[3 * i + 2], d[0], d[1], d[2]) + ps_d3(J[9 + 3 * i], J[9 + 3 * i + 1], J[9 + 3 * i + 2], d[3], d[4], d[5]));
        yr[i] = wr * ps_d3(J[18 + 3 * i], J[18 + 3 * i + 1], J[18 + 3 * i + 2], d[3], d[4], d[5]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        u[j] = ps_d3(J[j], J[3 + j], J[6 + j], yt[0], yt[1], yt[2]);
        u[3 + j] = ps_d3(J[9 + j], J[12 + j], J[15 + j], yt[0], yt[1], yt[2]) + ps_d3(J[18 + j], J[21 + j], J[24 + j], yr[0], yr[1], yr[2]);
    }
}

// The lower Cholesky factor of D = J^T W J, packed by rows (Lc[i (i + 1) / 2 + j]); false where a pivot is not > 0.
__device__ __forceinline__ bool rx_factor(const double (&J)[27], double wt, double wr, double (&Lc)[21]) {
#pragma clang fp contract(off)
    double U[21];                                      // D's upper triangle by rows
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double v;
            if (i < 3) {
                const int o = j < 3 ? j : 9 + (j - 3);
                v = wt * ps_d3(J[i], J[3 + i], J[6 + i], J[o], J[o + 3], J[o + 6]);
            } else {
                const int bi = 9 + (i - 3), bj = 9 + (j - 3), ci = 18 + (i - 3), cj = 18 + (j - 3);
                v = wt * ps_d3(J[bi], J[bi + 3], J[bi + 6], J[bj], J[bj + 3], J[bj + 6]) +
                    wr * ps_d3(J[ci], J[ci + 3], J[ci + 6], J[cj], J[cj + 3], J[cj + 6]);
            }
            U[i * (13 - i) / 2 + (j - i)] = v;
        }
    }
    return ps_chol6(U, Lc);
}

__device__ __forceinline__ double rx_leaf(const double (&x)[6], const double (&y)[6]) {
#pragma clang fp contract(off)
    return ((((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]) + x[3] * y[3]) + x[4] * y[4]) + x[5] * y[5];
}

// R <- C(w) R, c <- C(w) c + rho
__device__ __forceinline__ void rx_retract(const double (&eta)[6], double (&R)[9], double (&c)[3]) {
#pragma clang fp contract(off)
    double C[9], Rn[9], cn[3];
    ps_rotation<3>(1.0, 0.5 * eta[3], 0.5 * eta[4], 0.5 * eta[5], C);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = ps_d3(C[3 * i], C[3 * i + 1], C[3 * i + 2], R[j], R[3 + j], R[6 + j]);
        cn[i] = ps_d3(C[3 * i], C[3 * i + 1], C[3 * i + 2], c[0], c[1], c[2]) + eta[i];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = cn[k];
}

// ---- the two normative orders, per workgroup of 256 ------------------------------------------------------------------------------------
// Inclusive scan of one 6-vector per thread: eight Kogge-Stone steps, each reading the previous step's values (two LDS buffers, [k][256]:
// consecutive lanes read consecutive doubles).  The final values are also left in buffer 0; the caller's next use of `lds` is safe
// behind the leading barrier here.
__device__ __forceinline__ void rx_scan6(double (&v)[6], double* lds) {
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; ++k) lds[k * RX_BLOCK + tid] = v[k];
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int off = 1; off < RX_BLOCK; off <<= 1) {
        if (tid >= off) {
#pragma unroll
            for (int k = 0; k < 6; ++k) v[k] = v[k] + lds[(cur * 6 + k) * RX_BLOCK + tid - off];
        }
        cur ^= 1;
#pragma unroll
        for (int k = 0; k < 6; ++k) lds[(cur * 6 + k) * RX_BLOCK + tid] = v[k];
        __syncthreads();
    }
}

// What lies before block `blk`: the block totals (tot[k][256], the first nb written) scanned the same way; +0.0 before block 0.
__device__ __forceinline__ void rx_before(const double* __restrict__ tot, int nb, int blk, double* lds, double (&before)[6]) {
    const int tid = threadIdx.x;
    double t[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = tid < nb ? tot[k * RX_MAX_BLOCKS + tid] : 0.0;
    rx_scan6(t, lds);
#pragma unroll
    for (int k = 0; k < 6; ++k) before[k] = blk > 0 ? lds[k * RX_BLOCK + blk - 1] : 0.0;
}

// The subtree of the workgroup's 256 leaves (thread order), in every thread.  `slot`: 4 doubles of LDS.
__device__ __forceinline__ double rx_tree(double v, double* slot) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}
// the tree over the at most 256 workgroup partials, +0.0 behind them
__device__ __forceinline__ double rx_finish_tree(const double* __restrict__ part, int nb, double* slot) {
    return rx_tree((int)threadIdx.x < nb ? part[threadIdx.x] : 0.0, slot);
}

template <int N>
__device__ __forceinline__ void rx_load(double (&v)[N], const double* __restrict__ buf, int i, int stride) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = RX_AT(buf, k, i, stride);
}
template <int N>
__device__ __forceinline__ void rx_store(const double (&v)[N], double* __restrict__ buf, int i, int stride) {
#pragma unroll
    for (int k = 0; k < N; ++k) RX_AT(buf, k, i, stride) = v[k];
}

// ---- prep ----------------------------------------------------------------------------------------------------------------------------------
// T_eff: the first pose with a non-finite word.  One workgroup.
__global__ __launch_bounds__(RX_BLOCK) void rx_teff_kernel(const double* __restrict__ poses, int T, int L, int32_t* __restrict__ flags,
                                                           int32_t* __restrict__ num_out) {
    __shared__ int part[4];
    int first = T;
    for (int n = threadIdx.x; n < T; n += RX_BLOCK) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 12; ++k) ok = ok && __builtin_isfinite(poses[(size_t)n * 12 + k]);
        if (!ok) first = min(first, n);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) first = min(first, __shfl_xor(first, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int te = min(min(part[0], part[1]), min(part[2], part[3]));
        flags[RX_TE] = te;
        flags[RX_FAIL] = 0;
        num_out[0] = te;
        if (L == 0) flags[RX_ACTIVE] = 0, flags[RX_USED] = 0, num_out[1] = 0;
    }
}

// the skip rules, a thread per loop
__global__ __launch_bounds__(RX_BLOCK) void rx_loops_kernel(const int32_t* __restrict__ pairs, const double* __restrict__ rel,
                                                            const double* __restrict__ weights, int L, const int32_t* __restrict__ flags,
                                                            int32_t* __restrict__ status) {
    const int e = blockIdx.x * RX_BLOCK + threadIdx.x;
    if (e >= L) return;
    const int te = flags[RX_TE];
    const int s = pairs[2 * (size_t)e], t = pairs[2 * (size_t)e + 1];
    const double wt = weights[2 * (size_t)e], wr = weights[2 * (size_t)e + 1];
    bool ok = s >= 0 && s < te && t >= 0 && t < te && s != t;
#pragma unroll
    for (int k = 0; k < 12; ++k) ok = ok && __builtin_isfinite(rel[(size_t)e * 12 + k]);
    ok = ok && __builtin_isfinite(wt) && __builtin_isfinite(wr) && wt >= 0.0 && wr >= 0.0 && (wt > 0.0 || wr > 0.0);
    status[e] = ok ? 0 : EPC_STATUS_NO_EDGE;
}

// How many used loops add or subtract at node n (g[target + 1] += u, g[source + 1] -= u): a thread per node over all L loops (the reads
// are wave-uniform).  Writes the exclusive prefix inside the block and the block's total; workgroup 0 also counts the used loops.
__global__ __launch_bounds__(RX_BLOCK) void rx_count_kernel(const int32_t* __restrict__ pairs, const int32_t* __restrict__ status, int T, int L,
                                                            int32_t* __restrict__ flags, int32_t* __restrict__ num_out,
                                                            int32_t* __restrict__ start, int32_t* __restrict__ count,
                                                            int32_t* __restrict__ blocktot) {
    __shared__ int slot[4];
    const int n = blockIdx.x * RX_BLOCK + threadIdx.x;
    const int te = flags[RX_TE];
    int cnt = 0;
    if (n >= 1 && n < te) {
        for (int e = 0; e < L; ++e) {
            if (status[e] == 0) cnt += (pairs[2 * (size_t)e + 1] + 1 == n ? 1 : 0) + (pairs[2 * (size_t)e] + 1 == n ? 1 : 0);
        }
    }
    int total;
    const int before = block_scan<4, int>(cnt, slot, total);
    if (n < T) start[n] = before, count[n] = cnt;
    if (threadIdx.x == 0) blocktot[blockIdx.x] = total;
    if (blockIdx.x == 0) {
        int used = 0;
        for (int e = threadIdx.x; e < L; e += RX_BLOCK) used += status[e] == 0 ? 1 : 0;
        int all;
        block_scan<4, int>(used, slot, all);
        if (threadIdx.x == 0) {
            flags[RX_USED] = all;
            flags[RX_ACTIVE] = all > 0 && te >= 2 ? 1 : 0;
            num_out[1] = all;
        }
    }
}

// The stable fill of every node's list (entry = 2 e for "add u_e", 2 e + 1 for "subtract u_e", ascending e), and the state: R, c = t - t_0
// and, for n >= 1, Z_n = X_{n-1}^-1 X_n.
__global__ __launch_bounds__(RX_BLOCK) void rx_fill_kernel(const double* __restrict__ poses, const int32_t* __restrict__ pairs,
                                                           const int32_t* __restrict__ status, int T, int L, const int32_t* __restrict__ flags,
                                                           const int32_t* __restrict__ blocktot, int32_t* __restrict__ start,
                                                           const int32_t* __restrict__ count, int32_t* __restrict__ entries,
                                                           double* __restrict__ R, double* __restrict__ c, double* __restrict__ Z) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * RX_BLOCK + threadIdx.x;
    const int te = flags[RX_TE];
    if (n >= T) return;
    int base = 0;
    for (int b = 0; b < (int)blockIdx.x; ++b) base += blocktot[b];
    int pos = base + start[n];
    start[n] = pos;
    if (n >= te) return;
    if (count[n] > 0) {
        for (int e = 0; e < L; ++e) {
            if (status[e] != 0) continue;
            if (pairs[2 * (size_t)e + 1] + 1 == n)
                entries[pos++] = 2 * e;
            else if (pairs[2 * (size_t)e] + 1 == n)
                entries[pos++] = 2 * e + 1;
        }
    }
    double Rb[9], cb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Rb[3 * i + j] = poses[(size_t)n * 12 + 4 * i + j];
        cb[i] = poses[(size_t)n * 12 + 4 * i + 3] - poses[4 * i + 3];
    }
    rx_store<9>(Rb, R, n, T);
    rx_store<3>(cb, c, n, T);
    if (n == 0) return;
    double Ra[9], dc[3], Zn[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Ra[3 * i + j] = poses[(size_t)(n - 1) * 12 + 4 * i + j];
        const double ca = poses[(size_t)(n - 1) * 12 + 4 * i + 3] - poses[4 * i + 3];
        dc[i] = cb[i] - ca;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Zn[4 * i + j] = ps_d3(Ra[i], Ra[3 + i], Ra[6 + i], Rb[j], Rb[3 + j], Rb[6 + j]);
        Zn[4 * i + 3] = ps_d3(Ra[i], Ra[3 + i], Ra[6 + i], dc[0], dc[1], dc[2]);
    }
    rx_store<12>(Zn, Z, n, T);
}

// ---- linearisation -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_BLOCK) void rx_lin_chain_kernel(const double* __restrict__ R, const double* __restrict__ c,
                                                                const double* __restrict__ Z, int T, double wt, double wr,
                                                                int32_t* __restrict__ flags, double* __restrict__ cJ, double* __restrict__ cb,
                                                                double* __restrict__ cL, double* __restrict__ part) {
    __shared__ double slot[4];
    if (!flags[RX_ACTIVE]) return;
    const int n = blockIdx.x * RX_BLOCK + threadIdx.x;
    const int te = flags[RX_TE];
    double leaf = 0.0;
    if (n >= 1 && n < te) {
        double Ra[9], Rb[9], ca[3], cbn[3], Zn[12], J[27], b[6], Lc[21];
        rx_load<9>(Ra, R, n - 1, T);
        rx_load<9>(Rb, R, n, T);
        rx_load<3>(ca, c, n - 1, T);
        rx_load<3>(cbn, c, n, T);
        rx_load<12>(Zn, Z, n, T);
        leaf = rx_linearise(Ra, Rb, ca, cbn, Zn, wt, wr, J, b);
        rx_store<27>(J, cJ, n, T);
        rx_store<6>(b, cb, n, T);
        if (!rx_factor(J, wt, wr, Lc)) flags[RX_FAIL] = 1;                           // every writer writes the same value
        rx_store<21>(Lc, cL, n, T);
    }
    const double sum = rx_tree(leaf, slot);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// a loop: a = target, b = source.  U takes J^T W r, the loop's piece of the gradient.
__global__ __launch_bounds__(RX_BLOCK) void rx_lin_loops_kernel(const double* __restrict__ R, const double* __restrict__ c, int T,
                                                                const int32_t* __restrict__ pairs, const double* __restrict__ rel,
                                                                const double* __restrict__ weights, const int32_t* __restrict__ status, int L,
                                                                const int32_t* __restrict__ flags, double* __restrict__ lJ,
                                                                double* __restrict__ U, double* __restrict__ chi2, double* __restrict__ part) {
    __shared__ double slot[4];
    if (!flags[RX_ACTIVE]) return;
    const int e = blockIdx.x * RX_BLOCK + threadIdx.x;
    double leaf = 0.0;
    if (e < L) {
        if (status[e] == 0) {
            const int a = pairs[2 * (size_t)e + 1], b = pairs[2 * (size_t)e];
            double Ra[9], Rb[9], ca[3], cbn[3], Ze[12], J[27], g[6];
            rx_load<9>(Ra, R, a, T);
            rx_load<9>(Rb, R, b, T);
            rx_load<3>(ca, c, a, T);
            rx_load<3>(cbn, c, b, T);
#pragma unroll
            for (int k = 0; k < 12; ++k) Ze[k] = rel[(size_t)e * 12 + k];
            leaf = rx_linearise(Ra, Rb, ca, cbn, Ze, weights[2 * (size_t)e], weights[2 * (size_t)e + 1], J, g);
            rx_store<27>(J, lJ, e, L);
            rx_store<6>(g, U, e, L);
            chi2[e] = leaf;
        } else {
            chi2[e] = epc_nan_f64();
        }
    }
    const double sum = rx_tree(leaf, slot);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// cost = tree(chain leaves) + tree(loop leaves): one workgroup finishes both trees
__global__ __launch_bounds__(RX_BLOCK) void rx_cost_kernel(const double* __restrict__ part_chain, int nb, const double* __restrict__ part_loops,
                                                           int nlb, const int32_t* __restrict__ flags, double* __restrict__ cost) {
    __shared__ double slot[4];
    if (!flags[RX_ACTIVE]) return;
    const double chain = rx_finish_tree(part_chain, nb, slot);
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = 16 * threadIdx.x + k;
        v[k] = i < nlb ? part_loops[i] : 0.0;
    }
#pragma unroll
    for (int w = 16; w > 1; w >>= 1) {
#pragma unroll
        for (int k = 0; k < w / 2; ++k) v[k] = v[2 * k] + v[2 * k + 1];
    }
    const double loops = rx_tree(v[0], slot);
    if (threadIdx.x == 0) cost[0] = chain + loops;
}

// ---- scans and the product ---------------------------------------------------------------------------------------------------------------
// `dead` (or NULL): the flag of the CG iteration this launch belongs to; a solve that has ended skips the work.
// block scan of v -> s, the block's total -> tot
__global__ __launch_bounds__(RX_BLOCK) void rx_scan_kernel(const double* __restrict__ v, int T, const int32_t* __restrict__ flags,
                                                           const int32_t* __restrict__ dead, double* __restrict__ s, double* __restrict__ tot) {
    __shared__ double lds[2 * 6 * RX_BLOCK];
    if (!flags[RX_ACTIVE] || (dead && *dead)) return;
    const int n = blockIdx.x * RX_BLOCK + threadIdx.x;
    double x[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = n < T ? RX_AT(v, k, n, T) : 0.0;
    rx_scan6(x, lds);
    if (n < T) rx_store<6>(x, s, n, T);
    if (threadIdx.x == RX_BLOCK - 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) tot[k * RX_MAX_BLOCKS + blockIdx.x] = x[k];
    }
}

// eta = before_block + s
__global__ __launch_bounds__(RX_BLOCK) void rx_eta_kernel(const double* __restrict__ s, const double* __restrict__ tot, int T,
                                                          const int32_t* __restrict__ flags, const int32_t* __restrict__ dead,
                                                          double* __restrict__ eta) {
    __shared__ double lds[2 * 6 * RX_BLOCK];
    if (!flags[RX_ACTIVE] || (dead && *dead)) return;
    const int n = blockIdx.x * RX_BLOCK + threadIdx.x;
    double before[6];
    rx_before(tot, gridDim.x, blockIdx.x, lds, before);
    if (n >= T) return;
#pragma unroll
    for (int k = 0; k < 6; ++k) RX_AT(eta, k, n, T) = before[k] + RX_AT(s, k, n, T);
}

// u_e = J_e^T W J_e (eta_b - eta_a)
__global__ __launch_bounds__(RX_BLOCK) void rx_loop_apply_kernel(const double* __restrict__ eta, int T, const int32_t* __restrict__ pairs,
                                                                 const double* __restrict__ weights, const int32_t* __restrict__ status, int L,
                                                                 const int32_t* __restrict__ flags, const int32_t* __restrict__ dead,
                                                                 const double* __restrict__ lJ, double* __restrict__ U) {
    if (!flags[RX_ACTIVE] || *dead) return;
    const int e = blockIdx.x * RX_BLOCK + threadIdx.x;
    if (e >= L || status[e] != 0) return;
    const int a = pairs[2 * (size_t)e + 1], b = pairs[2 * (size_t)e];
    double J[27], d[6], u[6];
    rx_load<27>(J, lJ, e, L);
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = RX_AT(eta, k, b, T) - RX_AT(eta, k, a, T);
    rx_apply(J, weights[2 * (size_t)e], weights[2 * (size_t)e + 1], d, u);
    rx_store<6>(u, U, e, L);
}

// g[n] from the node's list in ascending loop index, then its block scan -> s, tot
__global__ __launch_bounds__(RX_BLOCK) void rx_gather_kernel(const double* __restrict__ U, int L, const int32_t* __restrict__ start,
                                                             const int32_t* __restrict__ count, const int32_t* __restrict__ entries, int T,
                                                             const int32_t* __restrict__ flags, const int32_t* __restrict__ dead,
                                                             double* __restrict__ s, double* __restrict__ tot) {
    __shared__ double lds[2 * 6 * RX_BLOCK];
    if (!flags[RX_ACTIVE] || (dead && *dead)) return;
    const int n = blockIdx.x * RX_BLOCK + threadIdx.x;
    double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n >= 1 && n < flags[RX_TE]) {
        const int first = start[n], cnt = count[n];
        for (int i = 0; i < cnt; ++i) {
            const int ent = entries[first + i], e = ent >> 1;
            if (ent & 1) {
#pragma unroll
                for (int k = 0; k < 6; ++k) g[k] = g[k] - RX_AT(U, k, e, L);
            } else {
#pragma unroll
                for (int k = 0; k < 6; ++k) g[k] = g[k] + RX_AT(U, k, e, L);
            }
        }
    }
    rx_scan6(g, lds);
    if (n < T) rx_store<6>(g, s, n, T);
    if (threadIdx.x == RX_BLOCK - 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) tot[k * RX_MAX_BLOCKS + blockIdx.x] = g[k];
    }
}

// Opens a solve: gradient[n] = b_n + scan(g)[n]; r = -gradient, z = D^-1 r, p = z, x = 0; the partial of r . z; the solve is alive.
__global__ __launch_bounds__(RX_BLOCK) void rx_start_kernel(const double* __restrict__ sg, const double* __restrict__ tot, int T,
                                                            const int32_t* __restrict__ flags, const double* __restrict__ cb,
                                                            const double* __restrict__ cL, double* __restrict__ x, double* __restrict__ r,
                                                            double* __restrict__ p, double* __restrict__ z, double* __restrict__ part_rz,
                                                            int32_t* __restrict__ dead) {
    __shared__ double lds[2 * 6 * RX_BLOCK];
    __shared__ double slot[4];
    if (!flags[RX_ACTIVE]) return;
    const int n = blockIdx.x * RX_BLOCK + threadIdx.x;
    const int te = flags[RX_TE];
    double before[6];
    rx_before(tot, gridDim.x, blockIdx.x, lds, before);
    double rn[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, zn[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n >= 1 && n < te) {
        double Lc[21];
        rx_load<21>(Lc, cL, n, T);
#pragma unroll
        for (int k = 0; k < 6; ++k) rn[k] = -(RX_AT(cb, k, n, T) + (before[k] + RX_AT(sg, k, n, T)));
        ps_chol6_solve(Lc, rn, zn);
    }
    if (n < T) {
        const double zero[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        rx_store<6>(zero, x, n, T);
        rx_store<6>(rn, r, n, T);
        rx_store<6>(zn, z, n, T);
        rx_store<6>(zn, p, n, T);
    }
    const double sum = rx_tree(n < te ? rx_leaf(rn, zn) : 0.0, slot);
    if (threadIdx.x == 0) part_rz[blockIdx.x] = sum;
    if (blockIdx.x == 0 && threadIdx.x == 0) dead[0] = 0;
}

// Hp[n] = J_n^T W J_n p_n + (before_block + s_g[n]); the partial of p . Hp
__global__ __launch_bounds__(RX_BLOCK) void rx_product_kernel(const double* __restrict__ sg, const double* __restrict__ tot, int T,
                                                              const int32_t* __restrict__ flags, const int32_t* __restrict__ dead,
                                                              const double* __restrict__ cJ, double wt, double wr, const double* __restrict__ p,
                                                              double* __restrict__ hp, double* __restrict__ part_php) {
#pragma clang fp contract(off)
    __shared__ double lds[2 * 6 * RX_BLOCK];
    __shared__ double slot[4];
    if (!flags[RX_ACTIVE] || *dead) return;
    const int n = blockIdx.x * RX_BLOCK + threadIdx.x;
    const int te = flags[RX_TE];
    double before[6];
    rx_before(tot, gridDim.x, blockIdx.x, lds, before);
    double pn[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n >= 1 && n < te) {
        double J[27], v[6];
        rx_load<27>(J, cJ, n, T);
        rx_load<6>(pn, p, n, T);
        rx_apply(J, wt, wr, pn, v);
#pragma unroll
        for (int k = 0; k < 6; ++k) h[k] = v[k] + (before[k] + RX_AT(sg, k, n, T));
    } else if (n == 0 && te > 0) {
        rx_load<6>(pn, p, n, T);
    }
    if (n < T) rx_store<6>(h, hp, n, T);
    const double sum = rx_tree(n < te ? rx_leaf(pn, h) : 0.0, slot);
    if (threadIdx.x == 0) part_php[blockIdx.x] = sum;
}

// ---- CG ------------------------------------------------------------------------------------------------------------------------------------
// alpha = r.z / p.Hp, both trees finished here; x += alpha p, r -= alpha Hp, z = D^-1 r; the partial of the new r . z.  dead[0] is this
// iteration's flag on entry, dead[1] the next one's: set where p.Hp is not finite and > 0.
__global__ __launch_bounds__(RX_BLOCK) void rx_update_kernel(int T, const int32_t* __restrict__ flags, int32_t* __restrict__ dead,
                                                             const double* __restrict__ part_php, const double* __restrict__ part_rz,
                                                             const double* __restrict__ cL, const double* __restrict__ p,
                                                             const double* __restrict__ hp, double* __restrict__ x, double* __restrict__ r,
                                                             double* __restrict__ z, double* __restrict__ part_rz_new) {
#pragma clang fp contract(off)
    __shared__ double slot[4];
    if (!flags[RX_ACTIVE]) return;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (dead[0]) {
        if (first) dead[1] = 1;
        return;
    }
    const double php = rx_finish_tree(part_php, gridDim.x, slot);
    if (!(__builtin_isfinite(php) && php > 0.0)) {
        if (first) dead[1] = 1;
        return;
    }
    if (first) dead[1] = 0;
    const double rz = rx_finish_tree(part_rz, gridDim.x, slot);
    const double alpha = rz / php;
    const int n = blockIdx.x * RX_BLOCK + threadIdx.x;
    const int te = flags[RX_TE];
    double rn[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, zn[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n < te) {
        double xn[6], pn[6], hn[6];
        rx_load<6>(xn, x, n, T);
        rx_load<6>(pn, p, n, T);
        rx_load<6>(hn, hp, n, T);
        rx_load<6>(rn, r, n, T);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            xn[k] = xn[k] + alpha * pn[k];
            rn[k] = rn[k] - alpha * hn[k];
        }
        if (n >= 1) {
            double Lc[21];
            rx_load<21>(Lc, cL, n, T);
            ps_chol6_solve(Lc, rn, zn);
        }
        rx_store<6>(xn, x, n, T);
        rx_store<6>(rn, r, n, T);
        rx_store<6>(zn, z, n, T);
    }
    const double sum = rx_tree(n < te ? rx_leaf(rn, zn) : 0.0, slot);
    if (threadIdx.x == 0) part_rz_new[blockIdx.x] = sum;
}

// beta = (new r.z) / (old r.z); p = z + beta p
__global__ __launch_bounds__(RX_BLOCK) void rx_direction_kernel(int T, const int32_t* __restrict__ flags, const int32_t* __restrict__ dead_next,
                                                                const double* __restrict__ part_rz, const double* __restrict__ part_rz_new,
                                                                const double* __restrict__ z, double* __restrict__ p) {
#pragma clang fp contract(off)
    __shared__ double slot[4];
    if (!flags[RX_ACTIVE] || *dead_next) return;
    const double rz = rx_finish_tree(part_rz, gridDim.x, slot);
    const double rz_new = rx_finish_tree(part_rz_new, gridDim.x, slot);
    const double beta = rz_new / rz;
    const int n = blockIdx.x * RX_BLOCK + threadIdx.x;
    if (n >= flags[RX_TE]) return;
#pragma unroll
    for (int k = 0; k < 6; ++k) RX_AT(p, k, n, T) = RX_AT(z, k, n, T) + beta * RX_AT(p, k, n, T);
}

// ---- the step and the outputs ------------------------------------------------------------------------------------------------------------
// eta = scan(x) finished here; nodes 1 .. T_eff - 1 are retracted by it
__global__ __launch_bounds__(RX_BLOCK) void rx_retract_kernel(const double* __restrict__ s, const double* __restrict__ tot, int T,
                                                              const int32_t* __restrict__ flags, double* __restrict__ R, double* __restrict__ c) {
#pragma clang fp contract(off)
    __shared__ double lds[2 * 6 * RX_BLOCK];
    if (!flags[RX_ACTIVE]) return;
    const int n = blockIdx.x * RX_BLOCK + threadIdx.x;
    double before[6];
    rx_before(tot, gridDim.x, blockIdx.x, lds, before);
    if (n < 1 || n >= flags[RX_TE]) return;
    double eta[6], Rn[9], cn[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) eta[k] = before[k] + RX_AT(s, k, n, T);
    rx_load<9>(Rn, R, n, T);
    rx_load<3>(cn, c, n, T);
    rx_retract(eta, Rn, cn);
    rx_store<9>(Rn, R, n, T);
    rx_store<3>(cn, c, n, T);
}

// poses_out; and, where nothing was solved or a pivot failed, the input copied through, every cost +0.0 and every chi2 NaN
__global__ __launch_bounds__(RX_BLOCK) void rx_finish_kernel(const double* __restrict__ poses, int T, int L, int iterations,
                                                             const int32_t* __restrict__ flags, const double* __restrict__ R,
                                                             const double* __restrict__ c, double* __restrict__ poses_out,
                                                             double* __restrict__ cost, double* __restrict__ chi2, int32_t* __restrict__ num_out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * RX_BLOCK + threadIdx.x;
    const int te = flags[RX_TE];
    const bool solved = flags[RX_ACTIVE] && !flags[RX_FAIL];
    if (i < T) {
        if (i >= te) {
#pragma unroll
            for (int k = 0; k < 12; ++k) poses_out[(size_t)i * 12 + k] = epc_nan_f64();
        } else if (!solved || i == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) poses_out[(size_t)i * 12 + k] = poses[(size_t)i * 12 + k];
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) poses_out[(size_t)i * 12 + 4 * a + b] = RX_AT(R, 3 * a + b, i, T);
                poses_out[(size_t)i * 12 + 4 * a + 3] = RX_AT(c, a, i, T) + poses[4 * a + 3];
            }
        }
    }
    if (!solved) {
        if (i < L) chi2[i] = epc_nan_f64();
        if (i <= iterations) cost[i] = 0.0;
        if (i == 0 && flags[RX_ACTIVE]) num_out[1] = -1;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
static bool rx_shape_ok(int T, int L) { return T >= 2 && T <= RX_MAX_T && L >= 0 && L <= RX_MAX_L; }

// The workspace.  float64, structure of arrays: R (9, T) c (3, T) Z (12, T) cJ (27, T) cb (6, T) cL (21, T) | x r p z hp eta sa sg (6, T)
// each | lJ (27, L) U (6, L) | tot_a tot_g (6, 256) | part_php (256) part_rz (2, 256) part_chain (256) part_loops (4096); int32: flags
// (4) dead (4098) start (T) count (T) blocktot (256) entries (2 L).
struct rx_ws {
    double *R, *c, *Z, *cJ, *cb, *cL, *x, *r, *p, *z, *hp, *eta, *sa, *sg, *lJ, *U, *tot_a, *tot_g, *part_php, *part_rz, *part_chain, *part_loops;
    int32_t *flags, *dead, *start, *count, *blocktot, *entries;
    size_t bytes;
};
static rx_ws rx_layout(void* base, int T, int L) {
    rx_ws w;
    epc_carver c(base);
    const size_t t = (size_t)T, l = (size_t)L;
    auto f64 = [&](size_t n) { return c.take<double>(n, 16); };
    auto i32 = [&](size_t n) { return c.take<int32_t>(n, 16); };
    w.R = f64(9 * t), w.c = f64(3 * t), w.Z = f64(12 * t), w.cJ = f64(27 * t), w.cb = f64(6 * t), w.cL = f64(21 * t);
    w.x = f64(6 * t), w.r = f64(6 * t), w.p = f64(6 * t), w.z = f64(6 * t), w.hp = f64(6 * t), w.eta = f64(6 * t), w.sa = f64(6 * t), w.sg = f64(6 * t);
    w.lJ = f64(27 * l), w.U = f64(6 * l);
    w.tot_a = f64(6 * RX_MAX_BLOCKS), w.tot_g = f64(6 * RX_MAX_BLOCKS);
    w.part_php = f64(RX_MAX_BLOCKS), w.part_rz = f64(2 * RX_MAX_BLOCKS), w.part_chain = f64(RX_MAX_BLOCKS), w.part_loops = f64(RX_MAX_LBLOCKS);
    w.flags = i32(RX_FLAGS), w.dead = i32(4096 + 2), w.start = i32(t), w.count = i32(t), w.blocktot = i32(RX_MAX_BLOCKS), w.entries = i32(2 * l);
    w.bytes = c.bytes();
    return w;
}

extern "C" size_t epcnet_trajectory_relax_workspace_bytes(int num_poses, int num_loops) {
    if (!rx_shape_ok(num_poses, num_loops)) return 0;
    return rx_layout(nullptr, num_poses, num_loops).bytes;
}

extern "C" int epcnet_trajectory_relax(const double* poses, int num_poses, const int32_t* pairs, const double* rel, const double* weights,
                                       int num_loops, double odo_w_t, double odo_w_r, int iterations, int cg_iterations, double* poses_out,
                                       double* cost, double* loop_chi2, int32_t* loop_status, int32_t* num_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    const int T = num_poses, L = num_loops;
    EPC_CHECK_ARG(rx_shape_ok(T, L), "need 2 <= num_poses <= 65536 and 0 <= num_loops <= 2^20");
    EPC_CHECK_ARG(poses && poses_out && cost && loop_chi2 && loop_status && num_out && workspace, "null pointer");
    EPC_CHECK_ARG(L == 0 || (pairs && rel && weights), "null pointer: pairs, rel and weights may be NULL only with num_loops == 0");
    EPC_CHECK_ARG(isfinite(odo_w_t) && odo_w_t > 0.0 && isfinite(odo_w_r) && odo_w_r > 0.0, "odo_w_t and odo_w_r must be finite and > 0");
    EPC_CHECK_ARG(iterations >= 0 && iterations <= 64, "need 0 <= iterations <= 64");
    EPC_CHECK_ARG(cg_iterations >= 1 && cg_iterations <= 4096, "need 1 <= cg_iterations <= 4096");
    EPC_CHECK_WORKSPACE(workspace, workspace_bytes, epcnet_trajectory_relax_workspace_bytes(T, L));
    const rx_ws w = rx_layout(workspace, T, L);
    hipStream_t st = (hipStream_t)stream;
    const int nb = rx_blocks(T), nlb = rx_blocks(L);
    const dim3 nodes(nb), loops(nlb), one(1), wg(RX_BLOCK);
    int32_t* const none = nullptr;

    hipLaunchKernelGGL(rx_teff_kernel, one, wg, 0, st, poses, T, L, w.flags, num_out);
    if (L > 0) {
        hipLaunchKernelGGL(rx_loops_kernel, loops, wg, 0, st, pairs, rel, weights, L, w.flags, loop_status);
        hipLaunchKernelGGL(rx_count_kernel, nodes, wg, 0, st, pairs, loop_status, T, L, w.flags, num_out, w.start, w.count, w.blocktot);
        hipLaunchKernelGGL(rx_fill_kernel, nodes, wg, 0, st, poses, pairs, loop_status, T, L, w.flags, w.blocktot, w.start, w.count, w.entries,
                           w.R, w.c, w.Z);
    }
    EPC_CHECK_LAUNCH();
    // with L == 0 nothing is solved: rx_teff_kernel has said so in the flags and only the finish runs
    for (int it = 0; L > 0 && it <= iterations; ++it) {
        hipLaunchKernelGGL(rx_lin_chain_kernel, nodes, wg, 0, st, w.R, w.c, w.Z, T, odo_w_t, odo_w_r, w.flags, w.cJ, w.cb, w.cL, w.part_chain);
        hipLaunchKernelGGL(rx_lin_loops_kernel, loops, wg, 0, st, w.R, w.c, T, pairs, rel, weights, loop_status, L, w.flags, w.lJ, w.U,
                           loop_chi2, w.part_loops);
        hipLaunchKernelGGL(rx_cost_kernel, one, wg, 0, st, w.part_chain, nb, w.part_loops, nlb, w.flags, cost + it);
        EPC_CHECK_LAUNCH();
        if (it == iterations) break;
        hipLaunchKernelGGL(rx_gather_kernel, nodes, wg, 0, st, w.U, L, w.start, w.count, w.entries, T, w.flags, none, w.sg, w.tot_g);
        hipLaunchKernelGGL(rx_start_kernel, nodes, wg, 0, st, w.sg, w.tot_g, T, w.flags, w.cb, w.cL, w.x, w.r, w.p, w.z, w.part_rz, w.dead);
        for (int k = 0; k < cg_iterations; ++k) {
            int32_t* dead = w.dead + k;
            double* rz = w.part_rz + (k & 1) * RX_MAX_BLOCKS;
            double* rz_new = w.part_rz + ((k + 1) & 1) * RX_MAX_BLOCKS;
            hipLaunchKernelGGL(rx_scan_kernel, nodes, wg, 0, st, w.p, T, w.flags, dead, w.sa, w.tot_a);
            hipLaunchKernelGGL(rx_eta_kernel, nodes, wg, 0, st, w.sa, w.tot_a, T, w.flags, dead, w.eta);
            hipLaunchKernelGGL(rx_loop_apply_kernel, loops, wg, 0, st, w.eta, T, pairs, weights, loop_status, L, w.flags, dead, w.lJ, w.U);
            hipLaunchKernelGGL(rx_gather_kernel, nodes, wg, 0, st, w.U, L, w.start, w.count, w.entries, T, w.flags, dead, w.sg, w.tot_g);
            hipLaunchKernelGGL(rx_product_kernel, nodes, wg, 0, st, w.sg, w.tot_g, T, w.flags, dead, w.cJ, odo_w_t, odo_w_r, w.p, w.hp,
                               w.part_php);
            hipLaunchKernelGGL(rx_update_kernel, nodes, wg, 0, st, T, w.flags, dead, w.part_php, rz, w.cL, w.p, w.hp, w.x, w.r, w.z, rz_new);
            hipLaunchKernelGGL(rx_direction_kernel, nodes, wg, 0, st, T, w.flags, dead + 1, rz, rz_new, w.z, w.p);
            EPC_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(rx_scan_kernel, nodes, wg, 0, st, w.x, T, w.flags, none, w.sa, w.tot_a);
        hipLaunchKernelGGL(rx_retract_kernel, nodes, wg, 0, st, w.sa, w.tot_a, T, w.flags, w.R, w.c);
        EPC_CHECK_LAUNCH();
    }
    const int most = T > L ? (T > iterations + 1 ? T : iterations + 1) : (L > iterations + 1 ? L : iterations + 1);
    hipLaunchKernelGGL(rx_finish_kernel, dim3(rx_blocks(most)), wg, 0, st, poses, T, L, iterations, w.flags, w.R, w.c, poses_out, cost, loop_chi2,
                       num_out);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}
