// Relations and training tuples from poses (include/epcnet_poses.h; numpy restatement in
// tests/tuples_ref.py) -- what the reference does offline with pandas + sklearn KDTree (generate_training_tuples_baseline.py:52-62,
// generate_test_sets.py:95-104) and per step with Python lists and sets (loading_pointclouds.py:102-168).  No list is stored: the poses
// (num x 2 float64, 350 KB at Oxford's 21 711 records: cache-resident) are streamed and every relation is decided from the
// coordinates when it is needed.
//
//   pose_radius_kernel       256 threads per query: count, or the ordered index list (ballot + wave counts: ascending by construction)
//   tuple_candidates_kernel  1024 threads per key: threshold of the C smallest (hash, id) among the negatives, ordered compaction
//   tuple_sample_kernel      1024 threads per key: the same threshold for the P positives and the Nn negatives, their <= 64 survivors
//                            ranked in LDS; the other negative is one min-reduction with the 1 + Nn positive tests per record
// The threshold of "the k smallest 64-bit values of a set": radix passes of 11 bits from the top, each one streaming pass over the
// poses into a 2048-bin LDS histogram (integer LDS atomics: order-independent), a block scan of the bins, the bin the k-th value falls
// in; it ends as soon as the values up to and including that bin are exactly k (at Oxford size: 2 passes, rarely 3).  The values are
// recomputed per pass (a subtraction pair, two products, five integer multiplies), never stored.
// float64 throughout, every operation rounded once (contract off), so numpy decides every relation alike.
#include "scan_common.h"
#include "../../include/epcnet_poses.h"

#define PT_THREADS 1024
#define PT_WAVES (PT_THREADS / 64)
#define PT_BITS 11
#define PT_BINS (1 << PT_BITS)
#define PT_MAX_NUM (1 << 24)
#define PR_THREADS 256
#define PR_WAVES (PR_THREADS / 64)
#define PT_NONE (~0ull)

struct pt_seed {
    uint32_t seed_lo, seed_hi, step_lo, step_hi;
};
// the state in front of the record id: hash(c) = epc_mix32(state ^ c)
__device__ __forceinline__ uint32_t pt_state(const pt_seed& sd, uint32_t key, uint32_t stream) {
    uint32_t s = epc_mix32(sd.seed_lo);
    s = epc_mix32(s ^ sd.seed_hi);
    s = epc_mix32(s ^ sd.step_lo);
    s = epc_mix32(s ^ sd.step_hi);
    s = epc_mix32(s ^ key);
    return epc_mix32(s ^ stream);
}
__device__ __forceinline__ unsigned long long pt_value(uint32_t state, int c) {
    return ((unsigned long long)epc_mix32(state ^ (uint32_t)c) << 32) | (unsigned long long)(uint32_t)c;
}
__device__ __forceinline__ double pt_d2(const double2& a, const double2& b) {
#pragma clang fp contract(off)
    const double dx = a.x - b.x, dy = a.y - b.y;
    const double xx = dx * dx, yy = dy * dy;
    return xx + yy;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Radius lists
// ---------------------------------------------------------------------------------------------------------------------------------
// padded == nullptr: lens only.  skip_self: database index q is not counted for query q (the positives of a record).
__global__ __launch_bounds__(PR_THREADS) void pose_radius_kernel(const double2* __restrict__ query, const double2* __restrict__ db,
                                                                 int num_db, double r2, int skip_self, int width,
                                                                 int32_t* __restrict__ lens, int32_t* __restrict__ padded,
                                                                 int32_t* __restrict__ status) {
    __shared__ int wsum[2][PR_WAVES];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double2 qp = query[q];
    int32_t* row = padded ? padded + (size_t)q * width : nullptr;
    int base = 0, it = 0;
    for (int c0 = 0; c0 < num_db; c0 += PR_THREADS, ++it) {        // (uniform: every thread takes every chunk)
        const int c = c0 + tid;
        const bool hit = c < num_db && !(skip_self && c == q) && pt_d2(db[c], qp) <= r2;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
        if (lane == 0) wsum[it & 1][wave] = __builtin_popcountll(mask);
        __syncthreads();       // (double-buffered: the chunk after the next one rewrites this half, one barrier later)
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PR_WAVES; ++w) {
            const int t = wsum[it & 1][w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (hit && row) {
            const int pos = base + before + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
            if (pos < width) row[pos] = c;
        }
        base += total;
    }
    if (row)
        for (int i = min(base, width) + tid; i < width; i += PR_THREADS) row[i] = -2;
    if (tid == 0) {
        lens[q] = base;
        if (row && base > width) atomicOr(status, 1);              // (only a truncated row: the sticky word of the call)
    }
}

static int pt_radius2(const double* radius, const char* who, double& r2) {
    if (!radius || !(*radius >= 0.0) || !(*radius * *radius <= 1.0e300)) {
        epc_set_error("%s: a radius is one finite double >= 0 in host memory", who);
        return EPC_EINVAL;
    }
    r2 = *radius * *radius;
    return EPC_OK;
}

static int pose_radius_launch(const char* who, const double* query, int num_q, const double* db, int num_db, const double* radius,
                              int skip_self, int width, int32_t* lens, int32_t* padded, int32_t* status, void* stream) {
    if (!query || !db || !lens || num_q < 0 || num_db < 0 || num_db > PT_MAX_NUM || !epc_aligned16(query) || !epc_aligned16(db)) {
        epc_set_error("%s: need 16-byte aligned poses, lens, num_q >= 0 and 0 <= num_db <= 2^24", who);
        return EPC_EINVAL;
    }
    double r2;
    if (int rc = pt_radius2(radius, who, r2)) return rc;
    if (num_q == 0) return EPC_OK;
    hipLaunchKernelGGL(pose_radius_kernel, dim3(num_q), dim3(PR_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const double2*>(query), reinterpret_cast<const double2*>(db), num_db, r2, skip_self, width, lens,
                       padded, status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        epc_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
        return EPC_EHIP;
    }
    return EPC_OK;
}

extern "C" int epcnet_pose_radius_count(const double* query, int num_q, const double* db, int num_db, const double* radius, int32_t* lens,
                                        void* stream) {
    return pose_radius_launch(__func__, query, num_q, db, num_db, radius, 0, 0, lens, nullptr, nullptr, stream);
}

extern "C" int epcnet_pose_radius_fill(const double* query, int num_q, const double* db, int num_db, const double* radius, int width,
                                       int32_t* lens, int32_t* padded, int32_t* status, void* stream) {
    EPC_CHECK_ARG(padded && status && width > 0, "need padded, status and width > 0");
    return pose_radius_launch(__func__, query, num_q, db, num_db, radius, 0, width, lens, padded, status, stream);
}

extern "C" int epcnet_pose_pos_count(const double* poses, int num, const double* r_pos, int32_t* counts, void* stream) {
    return pose_radius_launch(__func__, poses, num, poses, num, r_pos, 1, 0, counts, nullptr, nullptr, stream);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Tuples
// ---------------------------------------------------------------------------------------------------------------------------------
struct pt_shared {
    unsigned hist[PT_BINS];
    int scan[PT_WAVES];
    int wsum[2][PT_WAVES];
    unsigned long long wmin[PT_WAVES];
    int sel_bin, sel_before, sel_incl;
    int list_n, nneg;
    unsigned long long list[EPC_TUPLE_MAX_IDS];
    int sorted[EPC_TUPLE_MAX_IDS];
    int neg[EPC_TUPLE_MAX_IDS];
    double2 negpose[EPC_TUPLE_MAX_IDS];
};

// the positives of the key (c != key, within r_pos) / its negatives (strictly outside r_neg), with their values of one stream
struct pt_positive {
    const double2* poses;
    double2 kp;
    double r2;
    int key;
    uint32_t state;
    __device__ __forceinline__ bool operator()(int c, unsigned long long& v) const {
        v = pt_value(state, c);
        return c != key && pt_d2(poses[c], kp) <= r2;
    }
};
struct pt_negative {
    const double2* poses;
    double2 kp;
    double r2;
    uint32_t state;
    __device__ __forceinline__ bool operator()(int c, unsigned long long& v) const {
        v = pt_value(state, c);
        return pt_d2(poses[c], kp) > r2;
    }
};

// thr such that the members with value <= thr are exactly the min(k, #members) smallest; selected = that number.  k >= 1.
// Every thread of the workgroup calls it and gets the same answer.
template <class F>
__device__ __forceinline__ unsigned long long pt_threshold(const F& member, int num, int k, pt_shared& sh, int& selected) {
    const int tid = threadIdx.x;
    unsigned long long prefix = 0;     // the bits [hi, 64) of the k-th value
    int hi = 64, need = k;
    for (;;) {
        const int shift = hi > PT_BITS ? hi - PT_BITS : 0;
        const unsigned digit_mask = (1u << (hi - shift)) - 1u;
        for (int i = tid; i < PT_BINS; i += PT_THREADS) sh.hist[i] = 0u;
        __syncthreads();
        for (int c = tid; c < num; c += PT_THREADS) {
            unsigned long long v;
            if (member(c, v) && (hi == 64 || (v >> hi) == (prefix >> hi))) atomicAdd(&sh.hist[(unsigned)(v >> shift) & digit_mask], 1u);
        }
        __syncthreads();
        const int h0 = (int)sh.hist[2 * tid], h1 = (int)sh.hist[2 * tid + 1];
        int total;
        const int before = block_scan<PT_WAVES>(h0 + h1, sh.scan, total);
        if (hi == 64 && total <= need) {       // fewer members than asked for: all of them
            selected = total;
            return PT_NONE;
        }
        if (before < need && need <= before + h0 + h1) {   // exactly one thread: the bins are a partition and total >= need >= 1
            const bool first = need <= before + h0;
            sh.sel_bin = 2 * tid + (first ? 0 : 1);
            sh.sel_before = first ? before : before + h0;
            sh.sel_incl = first ? before + h0 : before + h0 + h1;
        }
        __syncthreads();
        const int bin = sh.sel_bin, sel_before = sh.sel_before, sel_incl = sh.sel_incl;
        prefix |= (unsigned long long)bin << shift;
        if (sel_incl == need || shift == 0) {  // the values up to this bin are exactly the k smallest (at shift 0 a bin holds one value)
            selected = k;
            return shift ? prefix | ((1ull << shift) - 1ull) : prefix;
        }
        need -= sel_before;
        hi = shift;
    }
}

// the members with value <= thr (at most EPC_TUPLE_MAX_IDS of them), ascending by value -> sh.sorted[0 .. n) as record ids
template <class F>
__device__ __forceinline__ void pt_collect_sorted(const F& member, int num, unsigned long long thr, int n, pt_shared& sh) {
    const int tid = threadIdx.x;
    if (tid == 0) sh.list_n = 0;
    __syncthreads();
    for (int c = tid; c < num; c += PT_THREADS) {
        unsigned long long v;
        if (member(c, v) && v <= thr) {
            const int slot = atomicAdd(&sh.list_n, 1);
            if (slot < EPC_TUPLE_MAX_IDS) sh.list[slot] = v;
        }
    }
    __syncthreads();
    if (tid < n && tid < EPC_TUPLE_MAX_IDS) {
        const unsigned long long v = sh.list[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += sh.list[j] < v ? 1 : 0;
        sh.sorted[rank] = (int)(uint32_t)v;
    }
    __syncthreads();
}

__device__ __forceinline__ void pt_flag(int32_t* status, int32_t* flagged, int b, int key, int bits) {
    if (bits) {
        status[b] = status[b] | bits;          // (the slot's word belongs to this workgroup: no atomic)
        if (flagged) flagged[b] = key;
    }
}

__global__ __launch_bounds__(PT_THREADS) void tuple_candidates_kernel(const double2* __restrict__ poses, int num,
                                                                      const int32_t* __restrict__ keys, double rneg2, pt_seed sd,
                                                                      int max_cand, int32_t* __restrict__ cand,
                                                                      int32_t* __restrict__ cand_count, int32_t* __restrict__ status,
                                                                      int32_t* __restrict__ flagged) {
    __shared__ pt_shared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int key = keys[b];
    if (key < 0 || key >= num) {               // (uniform)
        if (tid == 0) {
            cand_count[b] = 0;
            pt_flag(status, flagged, b, key, EPC_TUPLE_BAD_KEY);
        }
        return;
    }
    const pt_negative member = {poses, poses[key], rneg2, pt_state(sd, (uint32_t)key, EPC_TUPLE_STREAM_CANDIDATES)};
    int selected;
    const unsigned long long thr = pt_threshold(member, num, max_cand, sh, selected);
    int32_t* row = cand + (size_t)b * max_cand;
    int base = 0, it = 0;
    for (int c0 = 0; c0 < num; c0 += PT_THREADS, ++it) {            // ordered compaction: ascending ids
        const int c = c0 + tid;
        unsigned long long v;
        const bool hit = c < num && member(c, v) && v <= thr;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
        if (lane == 0) sh.wsum[it & 1][wave] = __builtin_popcountll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PT_WAVES; ++w) {
            const int t = sh.wsum[it & 1][w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (hit) {
            const int pos = base + before + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
            if (pos < max_cand) row[pos] = c;
        }
        base += total;
    }
    if (tid == 0) cand_count[b] = min(selected, max_cand);
}

__global__ __launch_bounds__(PT_THREADS) void tuple_sample_kernel(const double2* __restrict__ poses, int num,
                                                                  const int32_t* __restrict__ keys, double rpos2, double rneg2,
                                                                  pt_seed sd, int P, int Nn, const int32_t* __restrict__ hard, int H,
                                                                  int32_t* __restrict__ ids, int32_t* __restrict__ status,
                                                                  int32_t* __restrict__ flagged) {
    __shared__ pt_shared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = 1 + P + Nn + 1;
    int32_t* out = ids + (size_t)b * W;
    const int key = keys[b];
    if (key < 0 || key >= num) {               // (uniform)
        if (tid < W) out[tid] = -1;
        if (tid == 0) pt_flag(status, flagged, b, key, EPC_TUPLE_BAD_KEY);
        return;
    }
    const double2 kp = poses[key];
    int bits = 0;

    // ---- positives ------------------------------------------------------------------------------------------------------------------
    if (P > 0) {
        const pt_positive member = {poses, kp, rpos2, key, pt_state(sd, (uint32_t)key, EPC_TUPLE_STREAM_POSITIVES)};
        int n;
        const unsigned long long thr = pt_threshold(member, num, P, sh, n);
        pt_collect_sorted(member, num, thr, n, sh);
        if (tid < P) out[1 + tid] = tid < n ? sh.sorted[tid] : -1;
        if (n < P) bits |= EPC_TUPLE_FEW_POSITIVES;
    }

    // ---- negatives: the hard ones first, then the fill --------------------------------------------------------------------------------
    if (tid == 0) {
        int nh = 0;
        for (int j = 0; j < H && nh < Nn; ++j) {
            const int h = hard[(size_t)b * H + j];
            bool take = h >= 0 && h < num;
            for (int i = 0; i < nh && take; ++i) take = sh.neg[i] != h;
            if (take) sh.neg[nh++] = h;
        }
        sh.nneg = nh;
    }
    __syncthreads();
    const int nhard = sh.nneg;
    if (nhard < Nn) {                          // (uniform)
        // the Nn smallest negatives hold the Nn - nhard smallest that are not hard ones: at most nhard of them are
        const pt_negative member = {poses, kp, rneg2, pt_state(sd, (uint32_t)key, EPC_TUPLE_STREAM_NEGATIVES)};
        int n;
        const unsigned long long thr = pt_threshold(member, num, Nn, sh, n);
        pt_collect_sorted(member, num, thr, n, sh);
        if (tid == 0) {
            int nn = nhard;
            for (int i = 0; i < n && nn < Nn; ++i) {
                const int c = sh.sorted[i];
                bool take = true;
                for (int j = 0; j < nhard && take; ++j) take = sh.neg[j] != c;
                if (take) sh.neg[nn++] = c;
            }
            sh.nneg = nn;
        }
        __syncthreads();
    }
    const int nneg = sh.nneg;
    if (tid < Nn) out[1 + P + tid] = tid < nneg ? sh.neg[tid] : -1;
    if (nneg < Nn) bits |= EPC_TUPLE_FEW_NEGATIVES;

    // ---- the other negative: a positive neither of the key nor of a chosen negative ------------------------------------------------------
    if (tid < nneg) sh.negpose[tid] = poses[sh.neg[tid]];
    __syncthreads();
    const uint32_t state = pt_state(sd, (uint32_t)key, EPC_TUPLE_STREAM_OTHER);
    unsigned long long best = PT_NONE;
    for (int c = tid; c < num; c += PT_THREADS) {
        const double2 p = poses[c];
        bool eligible = !(c != key && pt_d2(p, kp) <= rpos2);
        for (int j = 0; j < nneg && eligible; ++j) eligible = !(c != sh.neg[j] && pt_d2(p, sh.negpose[j]) <= rpos2);
        if (eligible) {
            const unsigned long long v = pt_value(state, c);
            best = v < best ? v : best;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o < best ? o : best;
    }
    if (lane == 0) sh.wmin[wave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PT_WAVES; ++w) best = sh.wmin[w] < best ? sh.wmin[w] : best;
        out[0] = key;
        out[1 + P + Nn] = best == PT_NONE ? -1 : (int)(uint32_t)best;
        if (best == PT_NONE) bits |= EPC_TUPLE_NO_OTHER;
        pt_flag(status, flagged, b, key, bits);
    }
}

static pt_seed pt_seed_of(long long seed, long long step) {
    const unsigned long long s = (unsigned long long)seed, t = (unsigned long long)step;
    return {(uint32_t)s, (uint32_t)(s >> 32), (uint32_t)t, (uint32_t)(t >> 32)};
}

extern "C" int epcnet_tuple_candidates(const double* poses, int num, const int32_t* keys, int num_keys, const double* r_neg, long long seed,
                                       long long step, int max_cand, int32_t* cand, int32_t* cand_count, int32_t* status,
                                       int32_t* flagged, void* stream) {
    EPC_CHECK_ARG(poses && keys && cand && cand_count && status, "null pointer");
    EPC_CHECK_ARG(epc_aligned16(poses), "poses must be 16-byte aligned");
    EPC_CHECK_ARG(num > 0 && num <= PT_MAX_NUM, "need 0 < num <= 2^24");
    EPC_CHECK_ARG(max_cand > 0 && max_cand <= EPC_TUPLE_MAX_CAND, "need 0 < max_cand <= 4096");
    EPC_CHECK_ARG(num_keys >= 0 && num_keys <= 65535, "need 0 <= num_keys <= 65535");
    double r2;
    if (int rc = pt_radius2(r_neg, __func__, r2)) return rc;
    if (num_keys == 0) return EPC_OK;
    hipLaunchKernelGGL(tuple_candidates_kernel, dim3(num_keys), dim3(PT_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const double2*>(poses), num, keys, r2, pt_seed_of(seed, step), max_cand, cand, cand_count, status,
                       flagged);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}

extern "C" int epcnet_tuple_sample(const double* poses, int num, const int32_t* keys, int num_keys, const double* r_pos, const double* r_neg,
                                   long long seed, long long step, int num_pos, int num_neg, const int32_t* hard, int num_hard, int32_t* ids,
                                   int32_t* status, int32_t* flagged, void* stream) {
    EPC_CHECK_ARG(poses && keys && ids && status, "null pointer");
    EPC_CHECK_ARG(epc_aligned16(poses), "poses must be 16-byte aligned");
    EPC_CHECK_ARG(num > 0 && num <= PT_MAX_NUM, "need 0 < num <= 2^24");
    EPC_CHECK_ARG(num_pos >= 0 && num_neg >= 0 && num_pos + num_neg + 2 <= EPC_TUPLE_MAX_IDS, "need P, Nn >= 0 and P + Nn + 2 <= 64");
    EPC_CHECK_ARG(num_hard >= 0 && num_hard <= EPC_TUPLE_MAX_HARD && (num_hard == 0 || hard), "need 0 <= H <= 32, and hard when H > 0");
    EPC_CHECK_ARG(num_keys >= 0 && num_keys <= 65535, "need 0 <= num_keys <= 65535");
    double rp2, rn2;
    if (int rc = pt_radius2(r_pos, __func__, rp2)) return rc;
    if (int rc = pt_radius2(r_neg, __func__, rn2)) return rc;
    if (num_keys == 0) return EPC_OK;
    hipLaunchKernelGGL(tuple_sample_kernel, dim3(num_keys), dim3(PT_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const double2*>(poses), num, keys, rp2, rn2, pt_seed_of(seed, step), num_pos, num_neg, hard,
                       num_hard, ids, status, flagged);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}
