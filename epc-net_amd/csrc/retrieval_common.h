// The pieces of the exact k-nearest search that more than one entry runs: ONE definition each, so that every entry under the bit-for-bit
// contract of epc_pairwise_topk -- its two forms and the mining form (retrieval.hip), the prefix search (revisit.hip) -- rounds and
// breaks ties alike.  Device functions only; the kernels that call them are thin.
#pragma once
#include "train_common.h"

#define RT_EXTRA 8          // candidates beyond k whose GEMM distances bracket the answer
#define RT_MAXC 64          // k + RT_EXTRA <= one lane per candidate

// exact squared distance sum_c (q_c - d_c)^2: sequential over c, one rounding per operation.  ONE definition for every kernel under the
// bit-for-bit contract of epc_pairwise_topk (the first form, the re-rank and the fallback of the workspace form, the mining distances,
// the prefix search)
__device__ __forceinline__ float exact_d2(const float* __restrict__ q, const float* __restrict__ row, int dim) {
    float acc = 0.f;
    for (int c = 0; c < dim; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(row + c);
        const float4 u = *reinterpret_cast<const float4*>(q + c);
        const float e0 = u.x - v.x, e1 = u.y - v.y, e2 = u.z - v.z, e3 = u.w - v.w;
        acc += e0 * e0;
        acc += e1 * e1;
        acc += e2 * e2;
        acc += e3 * e3;
    }
    return acc;
}

// lexicographic (value, index) minimum over the wave
__device__ __forceinline__ void wave_argmin(float& best, int& bi) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        if (ov < best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
}

// One wave: the k smallest of the `num` squared distances d2 (LDS; consumed) in ascending (value, position) order -> idx, dist of one
// query.  Fewer than k entries at a finite distance (NaN / Inf query or rows -- the descriptors of flagged clouds -- or num < k): no such
// neighbour, index -1 at distance +Inf.  `map` (optional): mapped[r] = map[idx[r]], -1 where idx[r] is -1 (the mining form's row ids).
__device__ __forceinline__ void topk_rounds(float* d2, int num, int k, int lane, int32_t* __restrict__ idx, float* __restrict__ dist,
                                            const int32_t* __restrict__ map, int32_t* __restrict__ mapped) {
    for (int r = 0; r < k; ++r) {
        float best = INFINITY;
        int bi = 0x7fffffff;
        for (int d = lane; d < num; d += 64) {
            const float v = d2[d];
            if (v < best) {  // ascending d within a lane: strict < keeps the lower index on ties
                best = v;
                bi = d;
            }
        }
        wave_argmin(best, bi);
        if (lane == 0) {
            idx[r] = bi < num ? bi : -1;
            dist[r] = sqrtf(best);
            if (map) mapped[r] = bi < num ? map[bi] : -1;
            if (bi < num) d2[bi] = INFINITY;
        }
        __syncthreads();
    }
}

// One wave: |x|^2 of one row, every lane four of every 256 components, then a butterfly sum (the same value on every lane).  The norms of
// the GEMM form's d2 = |q|^2 + |d|^2 - 2 q.d and of its proof's bound
__device__ __forceinline__ float wave_rownorm2(const float* __restrict__ xrow, int dim, int lane) {
    float s = 0.f;
    for (int c = lane * 4; c < dim; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xrow + c);
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// One wave's 64 x 64 part of S[q][d] = max(|q|^2 + |d|^2 - 2 q.d, 0) at (q0, d0): four 32x32 f32-MFMA accumulators.
// Both operands are row-major (rows, dim) with the row on the lane -- exactly the A[i][k] / B[k][j] lane layouts of
// v_mfma_f32_32x32x2_f32 when a lane reads a float4 along K (k = 8b + 4 (lane >> 5) + c for component c of block b), so the
// fragments come straight from global memory (L2): no LDS, 4 float4 loads per 16 MFMAs.  Rows q < nq against rows d < nd (the caller
// has checked q0 < nq and d0 < nd); row q of S starts at S + q * ld.
__device__ __forceinline__ void pairdist_wave_tile(const float* __restrict__ Q, const float* __restrict__ D, const float* __restrict__ qn,
                                                   const float* __restrict__ dn, int nq, int nd, int dim, float* __restrict__ S,
                                                   int ld, int q0, int d0, int lane) {
    const int j = lane & 31, h = lane >> 5;
    const float* a0 = Q + (size_t)min(q0 + j, nq - 1) * dim + 4 * h;
    const float* a1 = Q + (size_t)min(q0 + 32 + j, nq - 1) * dim + 4 * h;
    const float* b0 = D + (size_t)min(d0 + j, nd - 1) * dim + 4 * h;
    const float* b1 = D + (size_t)min(d0 + 32 + j, nd - 1) * dim + 4 * h;
    f32x16 acc[2][2];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = acc[0][1][r] = acc[1][0][r] = acc[1][1][r] = 0.f;
    for (int k = 0; k < dim; k += 8) {
        const float4 x0 = *reinterpret_cast<const float4*>(a0 + k), x1 = *reinterpret_cast<const float4*>(a1 + k);
        const float4 y0 = *reinterpret_cast<const float4*>(b0 + k), y1 = *reinterpret_cast<const float4*>(b1 + k);
        const float xa[4] = {x0.x, x0.y, x0.z, x0.w}, xb[4] = {x1.x, x1.y, x1.z, x1.w};
        const float ya[4] = {y0.x, y0.y, y0.z, y0.w}, yb[4] = {y1.x, y1.y, y1.z, y1.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            acc[0][0] = mfma32(xa[c], ya[c], acc[0][0]);
            acc[0][1] = mfma32(xa[c], yb[c], acc[0][1]);
            acc[1][0] = mfma32(xb[c], ya[c], acc[1][0]);
            acc[1][1] = mfma32(xb[c], yb[c], acc[1][1]);
        }
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const int d = d0 + 32 * tj + j;
            if (d >= nd) continue;
            const float dnv = dn[d];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = q0 + 32 * ti + mfma_row(r, h);
                if (q < nq) {
                    // rounding can leave a tiny negative value for coincident rows: 0; a NaN / Inf descriptor (a flagged cloud):
                    // +Inf, never selected -- as in the exact form, where a NaN distance never wins a comparison
                    const float v = (qn[q] + dnv) - 2.0f * acc[ti][tj][r];
                    S[(size_t)q * ld + d] = v >= 0.f ? (v <= 3.0e38f ? v : INFINITY) : (v < 0.f ? 0.f : INFINITY);
                }
            }
        }
}

// One wave, one query: the kc = min(k + RT_EXTRA, nd) smallest entries of its row `grow` (nd GEMM values) in (value, index) order, their
// exact distances, the k best of those -> idx[0 .. min(k, kc)), dist likewise; returns 1 (on lane 0) when the bracket does not prove the
// answer.  `srow`: the workgroup's dynamic LDS -- room for the row (rounded up to 4 words) when rows_in_lds, and 4 x 64 words behind it.
__device__ __forceinline__ int select_rerank_row(const float* __restrict__ grow, float* srow, const float* __restrict__ qrow,
                                                 const float* __restrict__ D, float qq, float dn_max, int nd, int dim, int k,
                                                 int rows_in_lds, int lane, int32_t* __restrict__ idx, float* __restrict__ dist) {
    const float* row = grow;
    if (rows_in_lds) {
        for (int d = lane; d < nd; d += 64) srow[d] = grow[d];
        __syncthreads();
        row = srow;
    }
    const int kc = min(k + RT_EXTRA, nd);
    float lv = -1.f;      // last selected (value, index): values are >= 0
    int li = -1;
    int my_cand = -1;
    float my_approx = 0.f;
    // ---- fast selection: a bound, one filtering scan, a rank over <= 64 survivors (instead of kc full scans) ----------
    // (1) every lane keeps the 4 smallest VALUES of its stride of the row (a 4-slot median network: 4 instructions per entry);
    // (2) U = the kc-th smallest of those 256 values -- the kc-th smallest of a SUBSET of the row, hence an upper bound of the
    //     row's kc-th smallest value;  (3) one more scan appends every finite (value, index) with value <= U to an LDS list:
    //     it holds the row's kc smallest entries, usually kc of them or a few more;  (4) with at most 64 survivors a rank by
    //     (value, index) puts the kc smallest on lanes 0 .. kc-1 in exactly the order the kc scans below would have found
    //     them.  More than 64 survivors (masses of ties) or fewer than kc finite entries: the scans below take over.
    bool fast_ok = false;
    {
        float* sv = srow + (rows_in_lds ? ((nd + 3) & ~3) : 0);          // [64] survivor values, [64] indices, [64] + [64] ranked
        int* si = reinterpret_cast<int*>(sv + 64);
        float* cv = sv + 128;
        int* ci = reinterpret_cast<int*>(sv + 192);
        float t0 = INFINITY, t1 = INFINITY, t2 = INFINITY, t3 = INFINITY;
        for (int d = lane; d < nd; d += 64) {
            const float v = row[d];
            t3 = __builtin_amdgcn_fmed3f(t2, t3, v);
            t2 = __builtin_amdgcn_fmed3f(t1, t2, v);
            t1 = __builtin_amdgcn_fmed3f(t0, t1, v);
            t0 = fminf(t0, v);
        }
        float U = INFINITY;
        for (int r = 0; r < kc; ++r) {
            float m = t0;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) m = fminf(m, __shfl_xor(m, off));
            U = m;
            if (!(m < INFINITY)) break;                                   // fewer than kc finite values among the candidates
            const unsigned long long holders = __builtin_amdgcn_ballot_w64(t0 == m);
            if (lane == __builtin_ctzll(holders)) t0 = t1, t1 = t2, t2 = t3, t3 = INFINITY;   // pop ONE holder per round
        }
        int total = 0;
        if (U < INFINITY) {
            for (int d0 = 0; d0 < nd; d0 += 64) {
                const int d = d0 + lane;
                const float v = d < nd ? row[d] : INFINITY;
                const bool hit = v <= U && v < INFINITY;
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
                if (mask) {
                    const int pos = total + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
                    if (hit && pos < 64) sv[pos] = v, si[pos] = d;
                    total += __builtin_popcountll(mask);
                }
            }
        }
        if (total >= kc && total <= 64) {
            __syncthreads();
            const float v = lane < total ? sv[lane] : INFINITY;
            const int d = lane < total ? si[lane] : 0x7fffffff;
            int rank = 0;
            for (int c = 0; c < total; ++c) {
                const float ov = sv[c];
                const int od = si[c];
                if (ov < v || (ov == v && od < d)) ++rank;
            }
            if (lane < total) cv[rank] = v, ci[rank] = d;
            __syncthreads();
            if (lane < kc) my_cand = ci[lane], my_approx = cv[lane];
            fast_ok = true;
        }
    }
    for (int r = 0; r < (fast_ok ? 0 : kc); ++r) {
        float best = INFINITY;
        int bi = 0x7fffffff;
        for (int d = lane; d < nd; d += 64) {
            const float v = row[d];
            const bool after = v > lv || (v == lv && d > li);
            if (after && v < best) {   // ascending d within a lane: strict < keeps the lower index on ties
                best = v;
                bi = d;
            }
        }
        wave_argmin(best, bi);
        lv = best;
        li = bi;
        if (lane == r) {
            my_cand = bi < nd ? bi : 0x7fffff00 + lane;   // fewer than kc finite rows: a unique invalid index that sorts last
            my_approx = best;
        }
    }
    // exact distances of the candidates, one per lane
    float e = INFINITY;
    if (lane < kc && my_cand < nd) e = exact_d2(qrow, D + (size_t)my_cand * dim, dim);
    if (!(e <= 3.0e38f)) e = INFINITY;   // NaN distance (NaN query): sorts last, like the comparisons of the exact form
    // rank by (exact, index) among the candidates
    int rank = 0;
    for (int c = 0; c < kc; ++c) {
        const float oe = __shfl(e, c);
        const int oi = __shfl(my_cand, c);
        if (lane < kc && (oe < e || (oe == e && oi < my_cand))) ++rank;
    }
    if (lane < kc && rank < k) {
        idx[rank] = my_cand < nd ? my_cand : -1;
        dist[rank] = sqrtf(e);
    }
    // Proof that no row r outside the candidates belongs to the answer.  Its GEMM value g_r is >= the last candidate's (m).
    // With u = 2^-24 and c = (dim + 3) u (first order; the constant below carries slack):
    //   |g_r - d2_r| <= c (sqrt(qn) + sqrt(dn_r))^2 =: E_r   (norms: <= dim u each; dot product: dim sequential f32
    //                   accumulations, |err| <= dim u sum|q_c d_c| <= dim u sqrt(qn dn_r); the two final additions: 2 u),
    //   exact form:     e_r >= d2_r (1 - c)                  (one rounding per difference, square and addition).
    // E_r needs a bound that does not know r.  (a) dn_r <= dn_max, the largest finite squared norm of the database (of any set of
    // rows that holds the row's nd: a larger dn_max only asks for more margin):
    // E_r <= c (sqrt(qn) + sqrt(dn_max))^2.  (b) norm-free: if sqrt(dn_r) <= 3 sqrt(qn), E_r <= 16 c qn; otherwise
    // sqrt(qn) + sqrt(dn_r) < 2 (sqrt(dn_r) - sqrt(qn)) <= 2 sqrt(d2_r), so E_r <= 4 c d2_r and d2_r >= m (1 - 4c):
    // E_r <= c (16 qn + 4 m) either way.  Both hold, so the smaller applies:
    //   e_r >= m - eps,   eps = c (min((sqrt(qn) + sqrt(dn_max))^2, 16 qn + 4 m) + m).
    // The answer stands when the k-th exact distance is STRICTLY below m - eps (an equal distance at a lower index would
    // win the tie).  A row whose GEMM value is +Inf (NaN / Inf descriptor) has no finite exact distance either and is
    // never part of an answer: m = +Inf means every finite row is a candidate, nothing to prove.
    float kth_exact = (lane < kc && rank == k - 1) ? e : -INFINITY;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) kth_exact = fmaxf(kth_exact, __shfl_xor(kth_exact, off));
    const float m = __shfl(my_approx, kc - 1);
    int f = 0;
    if (kc < nd && m < INFINITY) {
        const float c = 1.05f * (float)(dim + 8) * 5.9604645e-8f;
        const float sq = sqrtf(qq) + sqrtf(dn_max);
        const float eps = c * (fminf(sq * sq, 16.0f * qq + 4.0f * m) + m) + 1e-37f;
        f = !(kth_exact < m - eps);
    }
    return f;
}

// One wave, one query without proof: exact distances of the nd rows into `row` (the query's row of S), then k rounds of arg-min
__device__ __forceinline__ void exact_fallback_row(float* __restrict__ row, const float* __restrict__ qrow, const float* __restrict__ D,
                                                   int nd, int dim, int k, int lane, int32_t* __restrict__ idx,
                                                   float* __restrict__ dist) {
    for (int d = lane; d < nd; d += 64) {
        const float v = exact_d2(qrow, D + (size_t)d * dim, dim);
        row[d] = v <= 3.0e38f ? v : INFINITY;      // NaN / overflow: never selected (as in select_rerank_row)
    }
    __syncthreads();
    for (int r = 0; r < k; ++r) {
        float best = INFINITY;
        int bi = 0x7fffffff;
        for (int d = lane; d < nd; d += 64) {
            const float v = row[d];
            if (v < best) {
                best = v;
                bi = d;
            }
        }
        wave_argmin(best, bi);
        if (lane == 0) {
            // fewer than k rows at a finite distance: no such neighbour (-1, +Inf) -- bi is NOT a row then, never store through it
            idx[r] = bi < nd ? bi : -1;
            dist[r] = sqrtf(best);
            if (bi < nd) row[bi] = INFINITY;
        }
        __syncthreads();
    }
}
