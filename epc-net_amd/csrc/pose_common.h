// ONE definition of what the pose solvers share -- register.hip (epcnet_pair_register, point-to-point ICP), localize.hip
// (epcnet_scan_localize, point-to-plane ICP), relax.hip (epcnet_trajectory_relax, pose-graph Gauss-Newton): each under a bit-for-bit
// contract with a numpy restatement (tests/register_ref.py, localize_ref.py, relax_ref.py), which forbids a second copy of a float64
// sequence.  Two parts:
//   the once-rounded SE(3) arithmetic of all three: the three-term dot, the rotation of an unnormalised quaternion, the unpivoted 6 x 6
//   Cholesky packed by rows and its substitutions;
//   the seeded-ICP scaffold of the first two, templated on the number of sums (17 / 29) where it appears: the limits and the workspace,
//   the seed half of the prep kernels, the head (the lane's source row) and the tail (the chunk's sums) of the correspondence kernels,
//   the tree over the chunks, and the host's launch sequence.
// Device helpers are __forceinline__ and every float64 helper carries its own contract(off): a kernel's code is what it was with the
// piece written out.
//
// Deliberately NOT here: the two solve kernels' thread organisation (a thread per pair, a wave per scan: moving one onto the other is a
// speed change), and with it their seed's choice, seed copy and output block: as shared helpers these reschedule rg_solve_kernel (same
// registers and scratch, another instruction order), and a call of 5 pairs of 4096 rows, which is that kernel's latency, then measured
// outside the parent's own spread on an MI355X (profiles/r24_pose_refactor.json), so they stay written out in both files; the test of
// the run flag in front of ps_corr_row (register.hip fills its LDS between the two); rg_rotate (sf_rotate of surfel_common.h is the
// same rotation on nine named registers, not 4 x 4 arrays: two published definitions); Horn's matrix (register.hip), rx_linearise /
// rx_apply (relax.hip); the searches and the leaf formulas of the two correspondence kernels; lz_cell and the index kernels
// (localize.hip).  (epcnet_pairs.h is included for EPC_STATUS_NO_PAIR, the status ps_prep_item writes; relax.hip uses the arithmetic only.)
#pragma once
#include "scan_common.h"
#include "../../include/epcnet_pairs.h"

#include <float.h>

// ---- the arithmetic of the three definitions ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double ps_d3(double a0, double a1, double a2, double b0, double b1, double b2) {
#pragma clang fp contract(off)
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// The rotation of the unnormalised quaternion (w, x, y, z), row-major with rows STRIDE apart.  (The two Gauss-Newton retractions pass the
// literal 1.0 for w: 1.0 * z and 1.0 * 1.0 are exact.)
template <int STRIDE>
__device__ __forceinline__ void ps_rotation(double w, double x, double y, double z, double* C) {
#pragma clang fp contract(off)
    const double nn = ((w * w + x * x) + y * y) + z * z;
    const double u = 2.0 / nn;
    C[0] = 1.0 - u * (y * y + z * z);
    C[1] = u * (x * y - w * z);
    C[2] = u * (x * z + w * y);
    C[STRIDE] = u * (x * y + w * z);
    C[STRIDE + 1] = 1.0 - u * (x * x + z * z);
    C[STRIDE + 2] = u * (y * z - w * x);
    C[2 * STRIDE] = u * (x * z - w * y);
    C[2 * STRIDE + 1] = u * (y * z + w * x);
    C[2 * STRIDE + 2] = 1.0 - u * (x * x + y * y);
}

// The lower Cholesky factor, packed by rows (Lc[i (i + 1) / 2 + j]), of the symmetric D given as its upper triangle packed by rows:
// D[i][j], i >= j, is U[j (13 - j) / 2 + (i - j)].  Unpivoted; false where a pivot is not > 0.
__device__ __forceinline__ bool ps_chol6(const double* U, double (&Lc)[21]) {
#pragma clang fp contract(off)
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = U[j * (13 - j) / 2];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - Lc[j * (j + 1) / 2 + k] * Lc[j * (j + 1) / 2 + k];
        ok = ok && s > 0.0;
        const double piv = __dsqrt_rn(s);
        Lc[j * (j + 1) / 2 + j] = piv;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = U[j * (13 - j) / 2 + (i - j)];
#pragma unroll
            for (int k = 0; k < j; ++k) t = t - Lc[i * (i + 1) / 2 + k] * Lc[j * (j + 1) / 2 + k];
            Lc[i * (i + 1) / 2 + j] = t / piv;
        }
    }
    return ok;
}

// z = D^-1 r from the factor
__device__ __forceinline__ void ps_chol6_solve(const double (&Lc)[21], const double (&r)[6], double (&z)[6]) {
#pragma clang fp contract(off)
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = r[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - Lc[i * (i + 1) / 2 + k] * y[k];
        y[i] = s / Lc[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s = s - Lc[k * (k + 1) / 2 + i] * z[k];
        z[i] = s / Lc[i * (i + 1) / 2 + i];
    }
}

// ---- the seeded-ICP scaffold: an item is a pair of clouds (register.hip) or a scan (localize.hip) ---------------------------------------
#define PS_CHUNK 256           // source rows per workgroup of a correspondence kernel: one per thread
#define PS_MAX_N 4096          // the leaves of the summation tree
#define PS_MAX_CHUNKS (PS_MAX_N / PS_CHUNK)
#define PS_MAX_ITEMS (1 << 20)
#define PS_MAX_SEEDS 64
#define PS_STATE 4             // int32 per item: status (0 = still running), best seed, source rows, target rows (0 where there are none)

static inline int ps_chunks(int n) { return (n + PS_CHUNK - 1) / PS_CHUNK; }
static inline bool ps_shape_ok(int items, int seeds, int n) {
    return items >= 0 && items <= PS_MAX_ITEMS && seeds >= 1 && seeds <= PS_MAX_SEEDS && n >= 32 && n <= PS_MAX_N && n % 32 == 0;
}
// the gate on d2, float32 and finite
static inline float ps_gate2(double max_dist) {
    const float g = (float)(max_dist * max_dist);
    return g < FLT_MAX ? g : FLT_MAX;
}

// the workspace: sums (items, seeds, chunks, SUMS) f64 | cur (items, 12) f64 | state (items, 4) i32 | run_a (items, seeds) i32 | run_b
// (items) i32, each rounded up to 16 bytes
struct ps_ws { double *sums, *cur; int32_t *state, *run_a, *run_b; size_t bytes; };
template <int SUMS>
static inline ps_ws ps_layout(void* base, int items, int seeds, int n) {
    epc_carver c(base);
    const size_t I = (size_t)items;
    return {c.take<double>(I * seeds * ps_chunks(n) * SUMS, 16), c.take<double>(I * 12, 16), c.take<int32_t>(I * PS_STATE, 16),
            c.take<int32_t>(I * seeds, 16), c.take<int32_t>(I, 16), c.bytes()};
}

// The seed half of a prep kernel, called by every thread of the item's workgroup of 256 (two barriers).  rows: the thread's counts of the
// rows that are not absent, of COUNTS clouds; base_ok: what the item needs apart from a finite seed (uniform).  Writes run_a of stage A
// (base_ok and twelve finite seed words), the identity into cur where there are no seeds, and the item's state.
template <int COUNTS>
__device__ __forceinline__ void ps_prep_item(int item, bool base_ok, int (&rows)[COUNTS], const double* __restrict__ seeds, int num_seeds,
                                             int32_t* __restrict__ state, int32_t* __restrict__ run_a, double* __restrict__ cur) {
    static_assert(COUNTS == 1 || COUNTS == 2, "the state has two words for row counts");
    __shared__ int part[COUNTS][4];
    __shared__ int any_seed;
    const int tid = threadIdx.x;
    if (tid == 0) any_seed = 0;
    __syncthreads();
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < COUNTS; ++k) rows[k] += __shfl_xor(rows[k], off);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < COUNTS; ++k) part[k][tid >> 6] = rows[k];
    }
    if (tid < num_seeds) {
        bool ok = base_ok;
        if (seeds) {
            const double* __restrict__ m = seeds + ((size_t)item * num_seeds + tid) * 12;
#pragma unroll
            for (int c = 0; c < 12; ++c) ok = ok && __builtin_isfinite(m[c]);
        }
        run_a[(size_t)item * num_seeds + tid] = ok ? 1 : 0;
        if (ok) any_seed = 1;                          // every writer writes the same value
    }
    if (!seeds && tid < 12) cur[(size_t)item * 12 + tid] = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
    __syncthreads();
    if (tid == 0) {
        int32_t* st = state + (size_t)item * PS_STATE;
        st[0] = any_seed ? 0 : EPC_STATUS_NO_PAIR;
        st[1] = -1;
        const int* second = part[COUNTS - 1];
        st[2] = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
        st[3] = COUNTS == 2 ? (second[0] + second[1]) + (second[2] + second[3]) : 0;
    }
}

// The head of a correspondence workgroup, behind its own test of the run flag (0: the pass is not wanted, the workgroup returns and
// nothing is written; the test stays in the kernel because register.hip fills its LDS between the test and this row): the lane's row
// of the chunk, from src (n, 3): zeros and not present behind the cloud, not present where it is absent.
__device__ __forceinline__ void ps_corr_row(const float* __restrict__ src, int n, int chunk, float& sx, float& sy, float& sz, bool& present) {
    sx = sy = sz = 0.f;
    present = false;
    const int i = chunk * PS_CHUNK + threadIdx.x;
    if (i < n) {
        sx = src[3 * i], sy = src[3 * i + 1], sz = src[3 * i + 2];
        present = epc_finite3(sx, sy, sz);
    }
}

// The tail: the chunk's SUMS subtree sums of the lanes' leaves v, a lane-xor butterfly (xor 1, 2, .. 32 = adjacent pairing), then the
// four waves -> out[0 .. SUMS).  Every thread of the workgroup calls it (one barrier).
template <int SUMS>
__device__ __forceinline__ void ps_chunk_sums(double (&v)[SUMS], double (&part)[PS_CHUNK / 64][SUMS], double* __restrict__ out) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < SUMS; ++k) {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) v[k] += __shfl_xor(v[k], off);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < SUMS; ++k) part[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid < SUMS) out[tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
}

// sum k of one pass: the tree over the chunks, an absent chunk the leaf +0.0
template <int SUMS>
__device__ __forceinline__ double ps_finish_sum(const double* __restrict__ chunk_sums, int chunks, int k) {
    double v[PS_MAX_CHUNKS];
#pragma unroll
    for (int c = 0; c < PS_MAX_CHUNKS; ++c) v[c] = c < chunks ? chunk_sums[c * SUMS + k] : 0.0;
#pragma unroll
    for (int w = PS_MAX_CHUNKS; w > 1; w >>= 1) {
#pragma unroll
        for (int c = 0; c < w / 2; ++c) v[c] = v[2 * c] + v[2 * c + 1];
    }
    return v[0];
}

// ---- host: the launches behind the entry's prep launch ---------------------------------------------------------------------------------
// corr(seed_count, poses, run) launches the correspondence kernel on the grid (items, seed_count, chunks); solve(pass_seeds, select,
// solve, output) the solve kernel behind it.  `who` names the entry in a launch failure.
template <class Corr, class Solve>
static inline int ps_drive(const char* who, const double* seeds, int num_seeds, int iterations, const ps_ws& w, Corr corr, Solve solve) {
    const auto launched = [who]() {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return EPC_OK;
        epc_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
        return EPC_EHIP;
    };
    // stage A: a pass per seed (under cur, the identity, where there are no seeds), the choice, and the first solve
    corr(num_seeds, seeds ? seeds : w.cur, w.run_a);
    solve(num_seeds, 1, iterations > 0 ? 1 : 0, iterations > 0 ? 0 : 1);
    if (launched() != EPC_OK) return EPC_EHIP;
    // stage B's further passes, then the final pass: all under cur
    for (int it = 1; it <= iterations; ++it) {
        const int last = it == iterations;
        corr(1, w.cur, w.run_b);
        solve(1, 0, last ? 0 : 1, last);
        if (launched() != EPC_OK) return EPC_EHIP;
    }
    return EPC_OK;
}
