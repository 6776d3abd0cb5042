// Revisit search (include/epcnet_revisits.h): the exact k nearest database rows per query among an ADMISSIBLE PREFIX database[:p_i] that
// differs from query to query -- the rows at least min_travel behind the query along the trajectory.  The workspace form of
// epc_pairwise_topk (retrieval.hip) with three changes: p_i comes from a float64 binary search on the device; a workgroup of the distance
// GEMM whose database tile starts at or beyond the largest p of its 128 queries returns at once (a sorted self-search computes the lower
// triangle); selection, exact re-rank, proof and fallback run over row[:p_i].  The arithmetic is retrieval_common.h's, the one
// definition: row i is bit for bit epc_pairwise_topk_ws on database[:p_i].
//
// Launches per call: 2 row norms, 1 check, 1 prefix, then (GEMM, select, fallback) per pass.  Nothing is read back and nothing is
// memset: every word a kernel reads was written by an earlier kernel of the same call.
#include "retrieval_common.h"
#include "../../include/epcnet_revisits.h"

#include <math.h>

#define RV_MAX_ROWS (1 << 22)
#define RV_TILE 128          // queries per GEMM tile = per workgroup of the prefix kernel

__global__ __launch_bounds__(256) void rv_rownorm2_kernel(const float* __restrict__ x, int rows, int dim, float* __restrict__ out) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const float s = wave_rownorm2(x + (size_t)r * dim, dim, lane);
    if (lane == 0) out[r] = s;
}

// One workgroup: *fail = db_along holds a non-finite entry or decreases anywhere; *dn_max = the largest FINITE squared norm of the
// database rows (0 for none).  num_db <= 2^22: at most 4096 entries per thread.
__global__ __launch_bounds__(1024) void rv_check_kernel(const double* __restrict__ db_along, const float* __restrict__ dn, int num_db,
                                                        float* __restrict__ dn_max, int32_t* __restrict__ fail) {
    __shared__ float part[16];
    __shared__ int bad_any;
    if (threadIdx.x == 0) bad_any = 0;
    __syncthreads();
    float m = 0.f;
    int bad = 0;
    for (int i = threadIdx.x; i < num_db; i += 1024) {
        const double a = db_along[i];
        bad |= !isfinite(a);
        if (i > 0) bad |= a < db_along[i - 1];
        const float v = dn[i];
        if (v <= 3.0e38f) m = fmaxf(m, v);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    if (bad) bad_any = 1;                              // every writer writes the same value
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) m = fmaxf(m, part[w]);
        *dn_max = m;
        *fail = bad_any;
    }
}

// One thread per query, one workgroup per tile of RV_TILE queries: count[i] = p_i = #{j : db_along[j] <= q_along[i] - min_travel} (one
// float64 subtraction, a binary search in float64), or -1 for a non-finite q_along[i] or a failed call; tile_pmax = the tile's largest p
// (0 for none): the columns of the distance matrix the tile needs.
__global__ __launch_bounds__(RV_TILE) void rv_prefix_kernel(const double* __restrict__ db_along, int num_db, const double* __restrict__ q_along,
                                                            int num_q, double min_travel, const int32_t* __restrict__ fail,
                                                            int32_t* __restrict__ count, int32_t* __restrict__ tile_pmax) {
    __shared__ int part[RV_TILE / 64];
    const int i = blockIdx.x * RV_TILE + threadIdx.x;
    int p = -1;
    if (i < num_q && !*fail) {
        const double qa = q_along[i];
        if (isfinite(qa)) {
            const double t = qa - min_travel;
            int lo = 0, hi = num_db;                   // db_along[j] <= t for every j < lo, > t for every j >= hi
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (db_along[mid] <= t) lo = mid + 1; else hi = mid;
            }
            p = lo;
        }
    }
    if (i < num_q) count[i] = p;
    int m = max(p, 0);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) tile_pmax[blockIdx.x] = max(part[0], part[1]);
}

// The distance GEMM of one pass: pairdist_gemm_kernel's tiling, the columns of a query tile cut at its largest p.  Row stride ld.
__global__ __launch_bounds__(256) void rv_pairdist_kernel(const float* __restrict__ Q, const float* __restrict__ D,
                                                          const float* __restrict__ qn, const float* __restrict__ dn,
                                                          const int32_t* __restrict__ tile_pmax, int nq, int ld, int dim,
                                                          float* __restrict__ S) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.y * RV_TILE + (wave >> 1) * 64, d0 = blockIdx.x * 128 + (wave & 1) * 64;
    const int pm = min(tile_pmax[blockIdx.y], ld);     // <= num_db by construction; the min keeps the stores inside the row regardless
    if (q0 >= nq || d0 >= pm) return;
    pairdist_wave_tile(Q, D, qn, dn, nq, pm, dim, S, ld, q0, d0, lane);
}

// One wave per query: select_rerank_row over row[:p]; a query with p <= 0 (nothing admissible, no answer by rule, failed call) writes
// its (-1, +Inf) row without touching the matrix; positions >= p of a short prefix are filled likewise.
__global__ __launch_bounds__(64) void rv_select_kernel(const float* __restrict__ S, const float* __restrict__ Q, const float* __restrict__ D,
                                                       const float* __restrict__ qn, const float* __restrict__ dn_max,
                                                       const int32_t* __restrict__ count, int ld, int dim, int k, int rows_in_lds,
                                                       int32_t* __restrict__ idx, float* __restrict__ dist, int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) float srow[];
    const int lane = threadIdx.x, qi = blockIdx.x;
    const int p = min(count[qi], ld);
    int32_t* qidx = idx + (size_t)qi * k;
    float* qdist = dist + (size_t)qi * k;
    int f = 0;
    if (p > 0) f = select_rerank_row(S + (size_t)qi * ld, srow, Q + (size_t)qi * dim, D, qn[qi], *dn_max, p, dim, k, rows_in_lds, lane, qidx, qdist);
    for (int r = max(p, 0) + lane; r < k; r += 64) qidx[r] = -1, qdist[r] = INFINITY;
    if (lane == 0) flag[qi] = f;
}

// flagged queries only (their p exceeds k + RT_EXTRA): the exact search over the prefix
__global__ __launch_bounds__(64) void rv_fallback_kernel(float* __restrict__ S, const float* __restrict__ Q, const float* __restrict__ D,
                                                         const int32_t* __restrict__ count, int ld, int dim, int k,
                                                         const int32_t* __restrict__ flag, int32_t* __restrict__ idx, float* __restrict__ dist) {
    const int lane = threadIdx.x, qi = blockIdx.x;
    if (!flag[qi]) return;
    exact_fallback_row(S + (size_t)qi * ld, Q + (size_t)qi * dim, D, min(count[qi], ld), dim, k, lane, idx + (size_t)qi * k, dist + (size_t)qi * k);
}

// queries per pass: the caller's, or the largest multiple of RV_TILE whose matrix stays below 1 GiB (at least one tile)
static int rv_pass(int num_db, int pass_queries) {
    if (pass_queries > 0) return pass_queries;
    long per = (1L << 28) / (num_db > 0 ? num_db : 1) / RV_TILE * RV_TILE;
    if (per < RV_TILE) per = RV_TILE;
    return (int)(per < RV_MAX_ROWS ? per : RV_MAX_ROWS);
}
static bool rv_shape_ok(int num_db, int num_q, int pass_queries) {
    return num_db >= 0 && num_db <= RV_MAX_ROWS && num_q >= 0 && num_q <= RV_MAX_ROWS &&
           (pass_queries == 0 || (pass_queries >= RV_TILE && pass_queries <= RV_MAX_ROWS && pass_queries % RV_TILE == 0));
}

// the workspace: S (min(ch, num_q), num_db) | dn (num_db) | qn (num_q) | flag (num_q) | tile_pmax (tiles) | dn_max and fail (a word each,
// one region), each region rounded up to 256 bytes; ch = queries per pass, tiles of RV_TILE queries
struct rv_ws { int ch, tiles; float *S, *dn, *qn; int32_t *flag, *tile_pmax; float* dn_max; int32_t* fail; size_t bytes; };
static rv_ws rv_layout(void* base, int num_db, int num_q, int pass_queries) {
    epc_carver c(base);
    const int ch = rv_pass(num_db, pass_queries), tiles = (num_q + RV_TILE - 1) / RV_TILE;
    rv_ws w = {ch, tiles, c.take<float>((size_t)(ch < num_q ? ch : num_q) * num_db, 256), c.take<float>(num_db, 256), c.take<float>(num_q, 256),
               c.take<int32_t>(num_q, 256), c.take<int32_t>(tiles, 256), c.take<float>(2, 256), nullptr, c.bytes()};
    if (w.dn_max) w.fail = reinterpret_cast<int32_t*>(w.dn_max + 1);
    return w;
}

extern "C" size_t epcnet_revisit_workspace_bytes(int num_db, int num_q, int pass_queries) {
    return rv_shape_ok(num_db, num_q, pass_queries) ? rv_layout(nullptr, num_db, num_q, pass_queries).bytes : 0;
}

extern "C" int epcnet_revisit_search(const float* database, const double* db_along, int num_db, const float* queries, const double* q_along,
                                     int num_q, int dim, double min_travel, int k, int pass_queries, int32_t* idx, float* dist,
                                     int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG(database && db_along && queries && q_along && idx && dist && count && workspace, "null pointer");
    EPC_CHECK_ARG(epc_aligned16(database) && epc_aligned16(queries) && epc_aligned16(workspace),
                  "database, queries and the workspace must be 16-byte aligned");
    EPC_CHECK_ARG(dim > 0 && dim % 8 == 0, "descriptor dim must be a multiple of 8");
    EPC_CHECK_ARG(k > 0 && k + RT_EXTRA <= RT_MAXC, "need 0 < k <= 56");
    EPC_CHECK_ARG(rv_shape_ok(num_db, num_q, pass_queries),
                  "need 0 <= num_db <= 2^22, 0 <= num_q <= 2^22, pass_queries 0 or a multiple of 128 in [128, 2^22]");
    EPC_CHECK_ARG(isfinite(min_travel) && min_travel >= 0.0, "min_travel must be finite and >= 0");
    if (num_q == 0) return EPC_OK;
    if (workspace_bytes < epcnet_revisit_workspace_bytes(num_db, num_q, pass_queries)) {
        epc_set_error("epcnet_revisit_search: workspace too small");
        return EPC_ENOMEM;
    }
    const rv_ws w = rv_layout(workspace, num_db, num_q, pass_queries);
    const int ch = w.ch;
    hipStream_t st = (hipStream_t)stream;
    if (num_db > 0) hipLaunchKernelGGL(rv_rownorm2_kernel, dim3((num_db + 3) / 4), dim3(256), 0, st, database, num_db, dim, w.dn);
    hipLaunchKernelGGL(rv_rownorm2_kernel, dim3((num_q + 3) / 4), dim3(256), 0, st, queries, num_q, dim, w.qn);
    hipLaunchKernelGGL(rv_check_kernel, dim3(1), dim3(1024), 0, st, db_along, w.dn, num_db, w.dn_max, w.fail);
    hipLaunchKernelGGL(rv_prefix_kernel, dim3(w.tiles), dim3(RV_TILE), 0, st, db_along, num_db, q_along, num_q, min_travel, w.fail, count,
                       w.tile_pmax);
    EPC_CHECK_LAUNCH();
    const int in_lds = (size_t)num_db * 4 <= 149 * 1024;
    const size_t lds_bytes = (in_lds ? (((size_t)num_db + 3) & ~(size_t)3) * 4 : 0) + 4 * 64 * 4;   // the row (if it fits) + the selection's 4 x 64 words
    EPC_SET_DYN_LDS(rv_select_kernel, 150 * 1024);
    for (int q0 = 0; q0 < num_q; q0 += ch) {
        const int nq = (num_q - q0) < ch ? (num_q - q0) : ch;
        const float* Qc = queries + (size_t)q0 * dim;
        if (num_db > 0)
            hipLaunchKernelGGL(rv_pairdist_kernel, dim3((num_db + 127) / 128, (nq + RV_TILE - 1) / RV_TILE), dim3(256), 0, st, Qc, database,
                               w.qn + q0, w.dn, w.tile_pmax + q0 / RV_TILE, nq, num_db, dim, w.S);
        hipLaunchKernelGGL(rv_select_kernel, dim3(nq), dim3(64), lds_bytes, st, w.S, Qc, database, w.qn + q0, w.dn_max, count + q0, num_db, dim, k,
                           in_lds, idx + (size_t)q0 * k, dist + (size_t)q0 * k, w.flag + q0);
        hipLaunchKernelGGL(rv_fallback_kernel, dim3(nq), dim3(64), 0, st, w.S, Qc, database, count + q0, num_db, dim, k, w.flag + q0,
                           idx + (size_t)q0 * k, dist + (size_t)q0 * k);
        EPC_CHECK_LAUNCH();
    }
    return EPC_OK;
}
