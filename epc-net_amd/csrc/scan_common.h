// ONE definition of what the scan front end shares -- downsample.hip, ground.hip, submap.hip, stamps.hip, pose_tuples.hip: the stages in
// front of the network, each under a bit-for-bit contract with a numpy restatement (tests/*_ref.py), so that a shared piece cannot drift
// between them.  Device helpers are __forceinline__: a kernel's code is what it was with the piece written out.
//
// Deliberately NOT here: sm_row / st_row and sm_pair_entry / st_pose_at (submap.hip, stamps.hip) -- their matrix layouts and the
// association of their float64 sums belong to two different published definitions --, and the two walks that list a tile's pairs (the
// submap's steps over slots as well as scans).
#pragma once
#include "common.h"

// the 32-bit mix of include/epcnet_poses.h (tests/tuples_ref.py, tests/ground_ref.py: mix)
__host__ __device__ __forceinline__ uint32_t epc_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ bool epc_finite3(float x, float y, float z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}
// the quiet NaN every stage writes for an absent row / an invalid pose
__device__ __forceinline__ float epc_nan_f32() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ double epc_nan_f64() { return __longlong_as_double(0x7ff8000000000000ll); }

// Exclusive prefix of v in thread order over a workgroup of WAVES waves; total = the workgroup's sum.  `slot` holds one word per wave.
// Integer T only: the result is exact whatever the order.  Two barriers: the first protects `slot` from the previous call's readers.
template <int WAVES, class T>
__device__ __forceinline__ T block_scan(T v, T* slot, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    __syncthreads();
    if (lane == 63) slot[wave] = incl;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const T t = slot[w];
        base += w < wave ? t : 0;
        total += t;
    }
    return base + incl - v;
}

// The first i in [lo, hi] with offsets[i + 1] > r: "the first scan whose end lies behind row r".  hi is returned when no i < hi
// qualifies -- a caller that knows a hit exists passes the last index, one that wants "none" passes the count.  offsets is
// non-decreasing over [lo, hi]; R is the caller's row type (int or long long).
template <class R>
__device__ __forceinline__ int first_scan_behind(const int32_t* __restrict__ offsets, int lo, int hi, R r) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((R)offsets[mid + 1] > r)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// The last pair of a tile's list that begins at or before `row`: p_out[0 .. np) ascending, p_out[0] <= row, np >= 1.
__device__ __forceinline__ int pair_of_row(const int* p_out, int np, int row) {
    int lo = 0, hi = np - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p_out[mid] <= row)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The offsets' rule -- offsets[0] >= 0, non-decreasing, offsets[num_scans] <= num_rows -- as the predicate of index i: the OR over
// i in [0, max(num_scans, 1)) is the rule's failure.  Every check keeps its own reduction and its own extra conditions.
template <class I>
__device__ __forceinline__ bool offsets_rule_bad(const int32_t* __restrict__ offsets, int num_scans, long long num_rows, I i) {
    bool bad = false;
    if (i == 0) bad = offsets[0] < 0 || (long long)offsets[num_scans] > num_rows;
    if (i < num_scans) bad |= offsets[i] > offsets[i + 1];
    return bad;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// Clears `count` <= 64 words in front of a call's other launches.  A kernel, not hipMemsetAsync: seen on an MI355X, a memset node of a
// captured graph wrote other bytes than its value from the second replay on (tests/test_gpu_stamps.py and tests/test_gpu_submap.py
// replay their graphs twice for this).  (static: every file that includes this header holds its own copy of these few instructions.)
static __global__ void scan_clear_words(int32_t* words, int count) {
    if ((int)threadIdx.x < count) words[threadIdx.x] = 0;
}
static inline int scan_clear_words_launch(int32_t* words, int count, void* stream, const char* who) {
    hipLaunchKernelGGL(scan_clear_words, dim3(1), dim3(64), 0, (hipStream_t)stream, words, count);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return EPC_OK;
    epc_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
    return EPC_EHIP;
}

// the refusal of a workspace that is too small, and, in front of it, of one that is not 16-byte aligned
// (_AS: under the name `who`, and of a buffer called `what`, a string literal -- growmap.hip's state is refused in the same words)
#define EPC_CHECK_BYTES_AS(who, what, bytes, need)                                                                    \
    do {                                                                                                             \
        if ((bytes) < (need)) {                                                                                      \
            epc_set_error("%s: " what " of %zu bytes, %zu needed", who, (size_t)(bytes), (size_t)(need));            \
            return EPC_ENOMEM;                                                                                       \
        }                                                                                                            \
    } while (0)
#define EPC_CHECK_WORKSPACE_BYTES(workspace_bytes, need) EPC_CHECK_BYTES_AS(__func__, "workspace", workspace_bytes, need)
#define EPC_CHECK_WORKSPACE_AS(who, workspace, workspace_bytes, need)                            \
    do {                                                                                         \
        EPC_CHECK_ARG_AS(who, epc_aligned16(workspace), "workspace must be 16-byte aligned");    \
        EPC_CHECK_BYTES_AS(who, "workspace", workspace_bytes, need);                             \
    } while (0)
#define EPC_CHECK_WORKSPACE(workspace, workspace_bytes, need) EPC_CHECK_WORKSPACE_AS(__func__, workspace, workspace_bytes, need)
