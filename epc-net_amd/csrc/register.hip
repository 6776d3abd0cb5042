// Pair registration (include/epcnet_pairs.h; numpy restatement in tests/register_ref.py): point-to-point ICP of P candidate pairs of
// clouds from caller-given seeds.  The definition is float32 distances in one association, float64 sums in ONE order (adjacent pairing
// over 4096 leaves indexed by source row), float64 Horn + Jacobi with every operation rounded once (contract off), so the result is the
// same bits on every run and equal to numpy's.
//
// pairs, seeds and the clouds are device data: every grid is sized from num_pairs, num_seeds and n alone, nothing is read back.
//   rg_prep_kernel     one workgroup per pair: the indices' range, the rows of both clouds that are not absent, which seeds are finite
//                      (or the identity where there are none); writes the pair's state and the run flags of stage A
//   rg_corr_kernel     the hot path, one per pass.  Grid (pair, seed, chunk of PS_CHUNK source rows): the target in LDS as three float
//                      arrays, +Inf in its absent rows (their d2 is +Inf and never wins: no mask in the loop); every lane keeps one
//                      transformed source row and reads four targets per wave-uniform 16-byte LDS read; packed float32 sub / mul / add on
//                      two targets at once (no FMA: the rounding of the definition), a compare and two selects per target; then the
//                      chunk's 17 subtree sums: a lane-xor butterfly (xor 1, 2, .. 32 = adjacent pairing), then the four waves
//   rg_solve_kernel    one thread per pair: finishes the tree over the chunks; after stage A chooses the seed; solves (Horn, cyclic
//                      Jacobi) for the next pass's pose; after the final pass writes the four outputs
// No atomics and no word read that an earlier kernel of the same call has not written: nothing to clear, no memset.
// What this file shares with localize.hip -- the limits, the workspace, the seeds' half of the prep kernel, the correspondence kernel's
// source row and chunk sums, the tree over the chunks, the host's launch sequence -- and the rotation of a quaternion are
// pose_common.h's (ps_*).
#include "pose_common.h"

#include <math.h>

#define RG_SUMS 17
#define RG_SWEEPS 6            // the header's count, fixed on the CPU

typedef float rg_f32x2 __attribute__((ext_vector_type(2)));

// ---- launch 1: the pairs -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rg_prep_kernel(const float* __restrict__ clouds, int num_clouds, int n, const int32_t* __restrict__ pairs,
                                                      const double* __restrict__ seeds, int num_seeds, int32_t* __restrict__ state,
                                                      int32_t* __restrict__ run_a, double* __restrict__ cur) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const int s = pairs[2 * p], t = pairs[2 * p + 1];
    const bool valid = s >= 0 && s < num_clouds && t >= 0 && t < num_clouds;
    int ns = 0, nt = 0;
    if (valid) {
        const float* __restrict__ src = clouds + (size_t)s * n * 3;
        const float* __restrict__ tgt = clouds + (size_t)t * n * 3;
        for (int i = tid; i < n; i += 256) {
            ns += epc_finite3(src[3 * i], src[3 * i + 1], src[3 * i + 2]) ? 1 : 0;
            nt += epc_finite3(tgt[3 * i], tgt[3 * i + 1], tgt[3 * i + 2]) ? 1 : 0;
        }
    }
    int rows[2] = {ns, nt};
    ps_prep_item(p, valid, rows, seeds, num_seeds, state, run_a, cur);
}

// ---- the correspondence pass -------------------------------------------------------------------------------------------------------------
// p_c of the definition: float64, every operation rounded once, one rounding to float32
__device__ __forceinline__ float rg_transform_row(const double* __restrict__ m, double x, double y, double z) {
#pragma clang fp contract(off)
    return (float)(((m[0] * x + m[1] * y) + m[2] * z) + m[3]);
}

// d2 of the definition for two targets at once, and the running minimum (ties and NaN keep the earlier row)
__device__ __forceinline__ void rg_two_targets(rg_f32x2 px, rg_f32x2 py, rg_f32x2 pz, rg_f32x2 qx, rg_f32x2 qy, rg_f32x2 qz, int j, float& best,
                                               int& bj) {
#pragma clang fp contract(off)
    const rg_f32x2 dx = px - qx, dy = py - qy, dz = pz - qz;
    const rg_f32x2 d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2.x < best) best = d2.x, bj = j;
    if (d2.y < best) best = d2.y, bj = j + 1;
}

// poses (num_pairs, num_seeds, 12); run (num_pairs, num_seeds): 0 = this pass is not wanted, nothing is written; sums (num_pairs, num_seeds,
// chunks, 17).  Grid (num_pairs, num_seeds, chunks), a chunk PS_CHUNK source rows.
__global__ __launch_bounds__(PS_CHUNK) void rg_corr_kernel(const float* __restrict__ clouds, int n, const int32_t* __restrict__ pairs,
                                                           const double* __restrict__ poses, const int32_t* __restrict__ run, float gate2,
                                                           double* __restrict__ sums) {
    __shared__ __attribute__((aligned(16))) float lx[PS_MAX_N];       // (three float arrays of the tree's leaves: 48 KB of LDS)
    __shared__ __attribute__((aligned(16))) float ly[PS_MAX_N];
    __shared__ __attribute__((aligned(16))) float lz[PS_MAX_N];
    __shared__ double part[PS_CHUNK / 64][RG_SUMS];
    const int p = blockIdx.x, h = blockIdx.y, chunk = blockIdx.z, tid = threadIdx.x;
    const size_t ph = (size_t)p * gridDim.y + h;
    if (!run[ph]) return;                              // (a run flag is only set for a pair whose indices are inside)
    const float* __restrict__ src = clouds + (size_t)pairs[2 * p] * n * 3;
    const float* __restrict__ tgt = clouds + (size_t)pairs[2 * p + 1] * n * 3;
    for (int j = tid; j < n; j += PS_CHUNK) {
        float x = tgt[3 * j], y = tgt[3 * j + 1], z = tgt[3 * j + 2];
        if (!epc_finite3(x, y, z)) x = y = z = INFINITY;
        lx[j] = x, ly[j] = y, lz[j] = z;
    }
    float sx, sy, sz;
    bool present;
    ps_corr_row(src, n, chunk, sx, sy, sz, present);
    const double* __restrict__ m = poses + ph * 12;
    const float nan = epc_nan_f32();
    const float px = present ? rg_transform_row(m, sx, sy, sz) : nan;
    const float py = present ? rg_transform_row(m + 4, sx, sy, sz) : nan;
    const float pz = present ? rg_transform_row(m + 8, sx, sy, sz) : nan;
    __syncthreads();
    float best = INFINITY;
    int bj = 0;
    if (chunk * PS_CHUNK + (tid & ~63) < n) {          // wave-uniform: a wave wholly behind the cloud has nothing to search
        const rg_f32x2 vx = {px, px}, vy = {py, py}, vz = {pz, pz};
        const float4* __restrict__ lx4 = reinterpret_cast<const float4*>(lx);
        const float4* __restrict__ ly4 = reinterpret_cast<const float4*>(ly);
        const float4* __restrict__ lz4 = reinterpret_cast<const float4*>(lz);
#pragma unroll 2
        for (int j4 = 0; j4 < n / 4; ++j4) {
            const float4 qx = lx4[j4], qy = ly4[j4], qz = lz4[j4];
            rg_two_targets(vx, vy, vz, rg_f32x2{qx.x, qx.y}, rg_f32x2{qy.x, qy.y}, rg_f32x2{qz.x, qz.y}, 4 * j4, best, bj);
            rg_two_targets(vx, vy, vz, rg_f32x2{qx.z, qx.w}, rg_f32x2{qy.z, qy.w}, rg_f32x2{qz.z, qz.w}, 4 * j4 + 2, best, bj);
        }
    }
    const bool acc = best <= gate2;                    // gate2 is finite: a lane that is not present (NaN) or found nothing (+Inf) fails
    double v[RG_SUMS];
    {
        const double a = acc ? 1.0 : 0.0;
        const double s0 = acc ? (double)sx : 0.0, s1 = acc ? (double)sy : 0.0, s2 = acc ? (double)sz : 0.0;
        const double q0 = acc ? (double)lx[bj] : 0.0, q1 = acc ? (double)ly[bj] : 0.0, q2 = acc ? (double)lz[bj] : 0.0;
        v[0] = a;
        v[1] = s0, v[2] = s1, v[3] = s2;
        v[4] = q0, v[5] = q1, v[6] = q2;
        v[7] = s0 * q0, v[8] = s0 * q1, v[9] = s0 * q2;                // exact: two float32 factors.  (A row that is not accepted is the
        v[10] = s1 * q0, v[11] = s1 * q1, v[12] = s1 * q2;             // leaf +0.0 in every sum: 0.0 * 0.0)
        v[13] = s2 * q0, v[14] = s2 * q1, v[15] = s2 * q2;
        v[16] = acc ? (double)best : 0.0;
    }
    ps_chunk_sums(v, part, sums + (ph * gridDim.z + chunk) * RG_SUMS);
}

// ---- the solve -----------------------------------------------------------------------------------------------------------------------------
// one Jacobi rotation of the pair (P, Q) on the symmetric a, accumulated into the eigenvectors e
template <int P, int Q>
__device__ __forceinline__ void rg_rotate(double (&a)[4][4], double (&e)[4][4]) {
#pragma clang fp contract(off)
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + __dsqrt_rn(theta * theta + 1.0));
    const double c = 1.0 / __dsqrt_rn(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    a[P][P] -= h;
    a[Q][Q] += h;
    a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double g = a[r][P], f = a[r][Q];
            a[r][P] = a[P][r] = c * g - s * f;
            a[r][Q] = a[Q][r] = s * g + c * f;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double g = e[r][P], f = e[r][Q];
        e[r][P] = c * g - s * f;
        e[r][Q] = s * g + c * f;
    }
}

// the pose of the 17 sums; false where it holds a non-finite word
__device__ __forceinline__ bool rg_solve(const double (&S)[RG_SUMS], double (&pose)[12]) {
#pragma clang fp contract(off)
    const double m = S[0];
    double M[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) M[a][b] = S[7 + 3 * a + b] - (S[1 + a] * S[4 + b]) / m;
    }
    double a[4][4], e[4][4];
    a[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    a[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    a[2][2] = (M[1][1] - M[0][0]) - M[2][2];
    a[3][3] = (M[2][2] - M[0][0]) - M[1][1];
    a[0][1] = a[1][0] = M[1][2] - M[2][1];
    a[0][2] = a[2][0] = M[2][0] - M[0][2];
    a[0][3] = a[3][0] = M[0][1] - M[1][0];
    a[1][2] = a[2][1] = M[0][1] + M[1][0];
    a[1][3] = a[3][1] = M[2][0] + M[0][2];
    a[2][3] = a[3][2] = M[1][2] + M[2][1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) e[r][c] = r == c ? 1.0 : 0.0;
    }
#pragma unroll 1
    for (int sweep = 0; sweep < RG_SWEEPS; ++sweep) {
        rg_rotate<0, 1>(a, e);
        rg_rotate<0, 2>(a, e);
        rg_rotate<0, 3>(a, e);
        rg_rotate<1, 2>(a, e);
        rg_rotate<1, 3>(a, e);
        rg_rotate<2, 3>(a, e);
    }
    double top = a[0][0], w = e[0][0], x = e[1][0], y = e[2][0], z = e[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        if (a[k][k] > top) top = a[k][k], w = e[0][k], x = e[1][k], y = e[2][k], z = e[3][k];
    }
    ps_rotation<4>(w, x, y, z, pose);
    const double sm0 = S[1] / m, sm1 = S[2] / m, sm2 = S[3] / m;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pose[4 * c + 3] = S[4 + c] / m - ((pose[4 * c] * sm0 + pose[4 * c + 1] * sm1) + pose[4 * c + 2] * sm2);
#pragma unroll
        for (int k = 0; k < 4; ++k) ok = ok && __builtin_isfinite(pose[4 * c + k]);
    }
    return ok;
}

// One thread per pair, behind a correspondence launch whose sums are (num_pairs, pass_seeds, chunks, 17).
//   select: the pass was stage A (pass_seeds = num_seeds): choose the seed, copy it to cur (where seeds is not NULL)
//   solve:  the next pose from the sums into cur, and run_b for the next pass
//   output: the pass was the final one: write pose, fit, info and status
__global__ __launch_bounds__(64) void rg_solve_kernel(const double* __restrict__ sums, int num_pairs, int pass_seeds, int chunks,
                                                      const double* __restrict__ seeds, const int32_t* __restrict__ run_a, int min_pairs,
                                                      int select, int solve, int output, int32_t* __restrict__ state,
                                                      int32_t* __restrict__ run_b, double* __restrict__ cur, double* __restrict__ pose_out,
                                                      double* __restrict__ fit_out, int32_t* __restrict__ info_out,
                                                      int32_t* __restrict__ status_out) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= num_pairs) return;
    int32_t* st = state + (size_t)p * PS_STATE;
    int status = st[0], best = st[1];
    double S[RG_SUMS], pose[12];
    double* mine = cur + (size_t)p * 12;
    if (status == 0) {
        int h = 0;
        if (select) {
            double bc = 0.0, bd = 0.0;
            best = -1;
            for (int k = 0; k < pass_seeds; ++k) {
                if (!run_a[(size_t)p * pass_seeds + k]) continue;
                const double* cs = sums + ((size_t)p * pass_seeds + k) * chunks * RG_SUMS;
                const double c = ps_finish_sum<RG_SUMS>(cs, chunks, 0), d = ps_finish_sum<RG_SUMS>(cs, chunks, 16);
                if (best < 0 || c > bc || (c == bc && d < bd)) best = k, bc = c, bd = d;
            }
            h = best;                                  // >= 0: status 0 says that a seed ran
            st[1] = best;
            if (seeds) {
#pragma unroll
                for (int c = 0; c < 12; ++c) mine[c] = seeds[((size_t)p * pass_seeds + h) * 12 + c];
            }
        }
        const double* cs = sums + ((size_t)p * pass_seeds + h) * chunks * RG_SUMS;
#pragma unroll
        for (int k = 0; k < RG_SUMS; ++k) S[k] = ps_finish_sum<RG_SUMS>(cs, chunks, k);
        if (S[0] < (double)min_pairs) {
            status = EPC_STATUS_NO_FIT;
        } else if (solve) {
            if (rg_solve(S, pose)) {
#pragma unroll
                for (int c = 0; c < 12; ++c) mine[c] = pose[c];
            } else {
                status = EPC_STATUS_NO_FIT;
            }
        }
        if (status) st[0] = status;
    }
    if (solve) run_b[p] = status == 0 ? 1 : 0;
    if (!output) return;
    const double nan = epc_nan_f64();
#pragma unroll
    for (int c = 0; c < 12; ++c) pose_out[(size_t)p * 12 + c] = status == 0 ? mine[c] : nan;
    {
#pragma clang fp contract(off)
        fit_out[2 * (size_t)p] = status == 0 ? S[16] / S[0] : nan;
        fit_out[2 * (size_t)p + 1] = status == 0 ? S[0] / (double)st[2] : nan;
    }
    info_out[4 * (size_t)p] = status == 0 ? best : -1;
    info_out[4 * (size_t)p + 1] = status == 0 ? (int)S[0] : 0;
    info_out[4 * (size_t)p + 2] = st[2];
    info_out[4 * (size_t)p + 3] = st[3];
    status_out[p] = status;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t epcnet_pair_register_workspace_bytes(int num_pairs, int num_seeds, int n) {
    return ps_shape_ok(num_pairs, num_seeds, n) ? ps_layout<RG_SUMS>(nullptr, num_pairs, num_seeds, n).bytes : 0;
}

extern "C" int epcnet_pair_register(const float* clouds, int num_clouds, int n, const int32_t* pairs, int num_pairs, const double* seeds,
                                    int num_seeds, double max_dist, int iterations, int min_pairs, double* pose, double* fit, int32_t* info,
                                    int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG(clouds && pairs && pose && fit && info && status && workspace, "null pointer");
    EPC_CHECK_ARG(epc_aligned16(clouds), "clouds must be 16-byte aligned");
    EPC_CHECK_ARG(ps_shape_ok(num_pairs, num_seeds, n) && num_clouds >= 1,
                  "need n a multiple of 32 in [32, 4096], num_clouds >= 1, 0 <= num_pairs <= 2^20, 1 <= num_seeds <= 64");
    EPC_CHECK_ARG(seeds || num_seeds == 1, "seeds is NULL: num_seeds must be 1 (the identity)");
    EPC_CHECK_ARG(isfinite(max_dist) && max_dist > 0.0, "max_dist must be finite and > 0");
    EPC_CHECK_ARG(iterations >= 0 && iterations <= 64, "need 0 <= iterations <= 64");
    EPC_CHECK_ARG(min_pairs >= 3 && min_pairs <= n, "need 3 <= min_pairs <= n");
    if (num_pairs == 0) return EPC_OK;
    EPC_CHECK_WORKSPACE(workspace, workspace_bytes, epcnet_pair_register_workspace_bytes(num_pairs, num_seeds, n));
    const float gate2 = ps_gate2(max_dist);
    const int chunks = ps_chunks(n);
    const ps_ws w = ps_layout<RG_SUMS>(workspace, num_pairs, num_seeds, n);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rg_prep_kernel, dim3(num_pairs), dim3(256), 0, st, clouds, num_clouds, n, pairs, seeds, num_seeds, w.state, w.run_a, w.cur);
    return ps_drive(
        __func__, seeds, num_seeds, iterations, w,
        [&](int seed_count, const double* poses, const int32_t* run) {
            hipLaunchKernelGGL(rg_corr_kernel, dim3(num_pairs, seed_count, chunks), dim3(PS_CHUNK), 0, st, clouds, n, pairs, poses, run, gate2,
                               w.sums);
        },
        [&](int pass_seeds, int select, int solve, int output) {
            hipLaunchKernelGGL(rg_solve_kernel, dim3((num_pairs + 63) / 64), dim3(64), 0, st, w.sums, num_pairs, pass_seeds, chunks, seeds, w.run_a,
                               min_pairs, select, solve, output, w.state, w.run_b, w.cur, pose, fit, info, status);
        });
}
