// Descriptor retrieval -- replaces sklearn KDTree(database).query(q, k=25) of evaluate.py:463,481.
//
// Two forms with identical results (exact k nearest rows by Euclidean distance, ties -> lower database index):
//   epc_pairwise_topk      no workspace: one wave per query, distances of the whole database in LDS (<= ~40 k rows);
//   epc_pairwise_topk_ws   the pairwise matrix as a tiled f32-MFMA GEMM (d2 = |q|^2 + |d|^2 - 2 q.d into the caller's
//                          workspace, any database size), per query the k + 8 smallest of its row, those candidates re-ranked
//                          by the EXACT sum_c (q_c - d_c)^2 the first form uses, and a proof per query that no other row can
//                          belong to the answer (the k-th exact distance lies below the last candidate's GEMM value by more
//                          than the GEMM's rounding bound); the rare query without proof (many near-ties) is redone exactly.
//
// First form: one wave per query.  Exact Euclidean distances sum_c (q_c - d_c)^2 in f32 (no ||q||^2+||d||^2-2q.d cancellation),
// kept in LDS; then k rounds of wave-wide arg-min (ties -> lower database index), so the result is the sorted
// k-nearest list.  Database sizes on this path are 10^2..10^4 rows (Oxford runs hold ~400 submaps each).
#include "retrieval_common.h"   // exact_d2, wave_argmin, topk_rounds and the workspace form's GEMM tile, selection and fallback

__global__ __launch_bounds__(64) void pairwise_topk_kernel(const float* __restrict__ db, int num_db,
                                                           const float* __restrict__ queries, int dim, int k,
                                                           int32_t* __restrict__ idx, float* __restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* qv = lds;          // dim
    float* d2 = lds + dim;    // num_db
    const int lane = threadIdx.x;
    const int qi = blockIdx.x;
    for (int c = lane; c < dim; c += 64) qv[c] = queries[(size_t)qi * dim + c];
    __syncthreads();
    for (int d = lane; d < num_db; d += 64) {
        const float acc = exact_d2(qv, db + (size_t)d * dim, dim);
        d2[d] = acc <= 3.0e38f ? acc : INFINITY;   // NaN / overflow: never selected
    }
    __syncthreads();
    topk_rounds(d2, num_db, k, lane, idx + (size_t)qi * k, dist + (size_t)qi * k, nullptr, nullptr);
}

extern "C" int epc_pairwise_topk(const float* database, int num_db, const float* queries, int num_q, int dim,
                                 int k, int32_t* idx, float* dist, void* stream) {
    EPC_CHECK_ARG(database && queries && idx && dist, "null pointer");
    EPC_CHECK_ARG(dim > 0 && dim % 4 == 0, "descriptor dim must be a multiple of 4");
    EPC_CHECK_ARG(k > 0 && k <= num_db, "need 0 < k <= num_db");
    EPC_CHECK_ARG(num_q >= 0, "bad shape");
    const size_t lds_bytes = ((size_t)dim + num_db) * sizeof(float);
    EPC_CHECK_ARG(lds_bytes <= 160 * 1024, "database shard too large for one LDS-resident pass (shard it)");
    if (num_q == 0) return EPC_OK;
    EPC_SET_DYN_LDS(pairwise_topk_kernel, lds_bytes);
    hipLaunchKernelGGL(pairwise_topk_kernel, dim3(num_q), dim3(64), lds_bytes, (hipStream_t)stream, database,
                       num_db, queries, dim, k, idx, dist);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}


// ---------------------------------------------------------------------------------------------------------------------
// Workspace form.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rownorm2_kernel(const float* __restrict__ x, int rows, int dim,
                                                       float* __restrict__ out) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const float s = wave_rownorm2(x + (size_t)r * dim, dim, lane);
    if (lane == 0) out[r] = s;
}

// S[q][d] = max(|q|^2 + |d|^2 - 2 q.d, 0): 128 x 128 tile per workgroup, 64 x 64 per wave (pairdist_wave_tile)
__global__ __launch_bounds__(256) void pairdist_gemm_kernel(const float* __restrict__ Q, const float* __restrict__ D,
                                                            const float* __restrict__ qn, const float* __restrict__ dn,
                                                            int nq, int nd, int dim, float* __restrict__ S) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.y * 128 + (wave >> 1) * 64, d0 = blockIdx.x * 128 + (wave & 1) * 64;
    if (q0 >= nq || d0 >= nd) return;
    pairdist_wave_tile(Q, D, qn, dn, nq, nd, dim, S, nd, q0, d0, lane);
}

// One wave per query: select_rerank_row over its whole row of S; flag[q] = 1 when the bracket does not prove the answer.
__global__ __launch_bounds__(64) void select_rerank_kernel(const float* __restrict__ S, const float* __restrict__ Q,
                                                           const float* __restrict__ D, const float* __restrict__ qn,
                                                           const float* __restrict__ dn_max, int nd, int dim, int k,
                                                           int rows_in_lds, int32_t* __restrict__ idx,
                                                           float* __restrict__ dist, int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) float srow[];
    const int lane = threadIdx.x, qi = blockIdx.x;
    const int f = select_rerank_row(S + (size_t)qi * nd, srow, Q + (size_t)qi * dim, D, qn[qi], *dn_max, nd, dim, k, rows_in_lds, lane,
                                    idx + (size_t)qi * k, dist + (size_t)qi * k);
    if (lane == 0) flag[qi] = f;
}

// largest FINITE squared norm of the database rows (one workgroup; nd is 10^2 .. 10^5)
__global__ __launch_bounds__(1024) void finite_max_kernel(const float* __restrict__ x, int n, float* __restrict__ out) {
    __shared__ float part[16];
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float v = x[i];
        if (v <= 3.0e38f) m = fmaxf(m, v);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) m = fmaxf(m, part[w]);
        *out = m;
    }
}

// flagged queries only: exact distances of the whole database into the query's row of S, then k rounds of arg-min
__global__ __launch_bounds__(64) void exact_fallback_kernel(float* __restrict__ S, const float* __restrict__ Q,
                                                            const float* __restrict__ D, int nd, int dim, int k,
                                                            const int32_t* __restrict__ flag, int32_t* __restrict__ idx,
                                                            float* __restrict__ dist) {
    const int lane = threadIdx.x, qi = blockIdx.x;
    if (!flag[qi]) return;
    exact_fallback_row(S + (size_t)qi * nd, Q + (size_t)qi * dim, D, nd, dim, k, lane, idx + (size_t)qi * k, dist + (size_t)qi * k);
}

// queries per pass: the pairwise matrix of one pass stays below 1 GiB
static int rt_chunk(int num_db, int num_q) {
    long per = (1L << 28) / (num_db > 0 ? num_db : 1);
    if (per < 128) per = 128;
    return (int)(per < num_q ? per : num_q);
}

// the workspace: S (ch, num_db) | dn (num_db) | qn (num_q) | flag (num_q) | dn_max (1), each rounded up to 256 bytes; ch = queries per pass
struct rt_ws { int ch; float *S, *dn, *qn; int32_t* flag; float* dn_max; size_t bytes; };
static rt_ws rt_layout(void* base, int num_db, int num_q) {
    epc_carver c(base);
    const int ch = rt_chunk(num_db, num_q);
    return {ch, c.take<float>((size_t)ch * num_db, 256), c.take<float>(num_db, 256), c.take<float>(num_q, 256), c.take<int32_t>(num_q, 256),
            c.take<float>(1, 256), c.bytes()};
}

extern "C" size_t epc_pairwise_topk_workspace_bytes(int num_db, int num_q) {
    return num_db > 0 && num_q > 0 ? rt_layout(nullptr, num_db, num_q).bytes : 0;
}

extern "C" int epc_pairwise_topk_ws(const float* database, int num_db, const float* queries, int num_q, int dim, int k,
                                    int32_t* idx, float* dist, void* workspace, size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG(database && queries && idx && dist && workspace, "null pointer");
    EPC_CHECK_ARG(dim > 0 && dim % 8 == 0, "descriptor dim must be a multiple of 8");
    EPC_CHECK_ARG(k > 0 && k <= num_db && k + RT_EXTRA <= RT_MAXC, "need 0 < k <= min(num_db, 56)");
    EPC_CHECK_ARG(num_q >= 0, "bad shape");
    if (num_q == 0) return EPC_OK;
    if (workspace_bytes < epc_pairwise_topk_workspace_bytes(num_db, num_q)) {
        epc_set_error("epc_pairwise_topk_ws: workspace too small");
        return EPC_ENOMEM;
    }
    const rt_ws w = rt_layout(workspace, num_db, num_q);
    const int ch = w.ch;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rownorm2_kernel, dim3((num_db + 3) / 4), dim3(256), 0, st, database, num_db, dim, w.dn);
    hipLaunchKernelGGL(rownorm2_kernel, dim3((num_q + 3) / 4), dim3(256), 0, st, queries, num_q, dim, w.qn);
    hipLaunchKernelGGL(finite_max_kernel, dim3(1), dim3(1024), 0, st, w.dn, num_db, w.dn_max);
    EPC_CHECK_LAUNCH();
    const int in_lds = (size_t)num_db * 4 <= 149 * 1024;
    const size_t lds_bytes = (in_lds ? (((size_t)num_db + 3) & ~(size_t)3) * 4 : 0) + 4 * 64 * 4;   // the row (if it fits) + the selection's 4 x 64 words
    EPC_SET_DYN_LDS(select_rerank_kernel, 150 * 1024);
    for (int q0 = 0; q0 < num_q; q0 += ch) {
        const int nq = (num_q - q0) < ch ? (num_q - q0) : ch;
        const float* Qc = queries + (size_t)q0 * dim;
        hipLaunchKernelGGL(pairdist_gemm_kernel, dim3((num_db + 127) / 128, (nq + 127) / 128), dim3(256), 0, st, Qc, database,
                           w.qn + q0, w.dn, nq, num_db, dim, w.S);
        hipLaunchKernelGGL(select_rerank_kernel, dim3(nq), dim3(64), lds_bytes, st, w.S, Qc, database, w.qn + q0, w.dn_max, num_db, dim, k,
                           in_lds, idx + (size_t)q0 * k, dist + (size_t)q0 * k, w.flag + q0);
        hipLaunchKernelGGL(exact_fallback_kernel, dim3(nq), dim3(64), 0, st, w.S, Qc, database, num_db, dim, k, w.flag + q0,
                           idx + (size_t)q0 * k, dist + (size_t)q0 * k);
        EPC_CHECK_LAUNCH();
    }
    return EPC_OK;
}


// ---------------------------------------------------------------------------------------------------------------------
// Mining form (train.py:857-869: KDTree over the sampled negatives' cached descriptors): every query against ITS OWN list of
// table rows, named by id.  Two launches: the distances, grid (candidate slabs, queries), one lane per candidate gathering its
// row from the table (so one query against 4000 rows is 63 workgroups' work, not one wave's); then one wave per query over the
// LDS copy of its distances -- topk_rounds, the selection of epc_pairwise_topk.
// ---------------------------------------------------------------------------------------------------------------------
#define MINE_SLAB 64
#define MINE_MAX_CAND 16384

__global__ __launch_bounds__(MINE_SLAB) void mine_dist_kernel(const float* __restrict__ table, int num_rows, int dim,
                                                              const float* __restrict__ queries, const int32_t* __restrict__ cand,
                                                              const int32_t* __restrict__ cand_count, int max_cand,
                                                              float* __restrict__ d2) {
    const int qi = blockIdx.y;
    const int count = min(max(cand_count[qi], 0), max_cand);
    const int p = blockIdx.x * MINE_SLAB + threadIdx.x;
    if (p >= count) return;
    const int id = cand[(size_t)qi * max_cand + p];
    float v = INFINITY;                                  // an id outside the table: never selected, nothing loaded
    if (id >= 0 && id < num_rows) {
        v = exact_d2(queries + (size_t)qi * dim, table + (size_t)id * dim, dim);
        if (!(v <= 3.0e38f)) v = INFINITY;               // NaN / overflow: never selected
    }
    d2[(size_t)qi * max_cand + p] = v;
}

__global__ __launch_bounds__(64) void mine_select_kernel(const float* __restrict__ d2, const int32_t* __restrict__ cand,
                                                         const int32_t* __restrict__ cand_count, int max_cand, int k,
                                                         int32_t* __restrict__ pos, int32_t* __restrict__ ids,
                                                         float* __restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x, qi = blockIdx.x;
    const int count = min(max(cand_count[qi], 0), max_cand);
    for (int d = lane; d < count; d += 64) lds[d] = d2[(size_t)qi * max_cand + d];
    __syncthreads();
    topk_rounds(lds, count, k, lane, pos + (size_t)qi * k, dist + (size_t)qi * k, cand + (size_t)qi * max_cand, ids + (size_t)qi * k);
}

extern "C" size_t epc_mine_topk_workspace_bytes(int num_q, int max_cand) {
    if (num_q <= 0 || max_cand <= 0) return 0;
    return epc_align_up((size_t)num_q * max_cand * sizeof(float), 256);
}

extern "C" int epc_mine_topk(const float* table, int num_rows, int dim, const float* queries, int num_q, const int32_t* cand,
                             const int32_t* cand_count, int max_cand, int k, int32_t* pos, int32_t* ids, float* dist, void* workspace,
                             size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG(table && queries && cand && cand_count && pos && ids && dist && workspace, "null pointer");
    EPC_CHECK_ARG(epc_aligned16(table) && epc_aligned16(queries), "table and queries must be 16-byte aligned");
    EPC_CHECK_ARG(dim > 0 && dim % 4 == 0, "descriptor dim must be a multiple of 4");
    EPC_CHECK_ARG(k > 0 && k + RT_EXTRA <= RT_MAXC, "need 0 < k <= 56");
    EPC_CHECK_ARG(num_rows > 0 && num_q >= 0 && num_q <= 65535 && max_cand > 0 && max_cand <= MINE_MAX_CAND,
                  "need num_rows > 0, 0 <= num_q <= 65535, 0 < max_cand <= 16384");
    if (num_q == 0) return EPC_OK;
    EPC_CHECK_ARG(workspace_bytes >= epc_mine_topk_workspace_bytes(num_q, max_cand), "workspace below epc_mine_topk_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    float* d2 = (float*)workspace;
    const size_t lds_bytes = (size_t)max_cand * sizeof(float);
    EPC_SET_DYN_LDS(mine_select_kernel, MINE_MAX_CAND * sizeof(float));
    hipLaunchKernelGGL(mine_dist_kernel, dim3((max_cand + MINE_SLAB - 1) / MINE_SLAB, num_q), dim3(MINE_SLAB), 0, st, table, num_rows, dim,
                       queries, cand, cand_count, max_cand, d2);
    hipLaunchKernelGGL(mine_select_kernel, dim3(num_q), dim3(64), lds_bytes, st, d2, cand, cand_count, max_cand, k, pos, ids, dist);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}
