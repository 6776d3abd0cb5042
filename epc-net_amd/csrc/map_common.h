// ONE definition of what the three voxel-map files share (map.hip: epcnet_map_fuse; surfel.hip: epcnet_map_surfels; growmap.hip:
// epcnet_surfel_map_add / _move) and that does not depend on a slot's layout beyond "the key is its first member": the bounds of a call's
// shape and their refusals, the row -> lattice step, the key of a cell and back, the hash, the claim loop and the read-only lookup of
// the open-addressing table, the words of the workspace's head, and the three levels of the leaders' scan.  What follows the slot --
// its sums, how rows are added to it, what is written from it -- is map.hip's own for its 40-byte slot and surfel_common.h's for the
// 128-byte one.  Device helpers are __forceinline__: a kernel's code is what it was with the piece written out.  (The tile prologue
// around mp_row is NOT here: it is surfel_common.h's sf_tile_row, and written out in map_insert_kernel -- DESIGN.md says why.)
#ifndef EPC_MAP_COMMON_H
#define EPC_MAP_COMMON_H
#include "scan_common.h"
#include "../../include/epcnet_maps.h"

#define MP_THREADS 256
#define MP_TILE 256            // rows per insert / count / emit tile, one per thread (tests/test_gpu_map.py names it MP_TILE)
#define MP_GROUP 256           // tiles per group: MP_TILE * MP_GROUP = 65536 rows is the scan's first level
#define MP_HEAD 16             // workspace words in front
#define MP_BAD 0               //   [0] the whole-call failure
#define MP_CLAIMED 1           //   [1] slots claimed
#define MP_KEPT 2              //   [2] rows kept, [3] rows absent, [4] rows out of range
#define MP_EMPTY 0xffffffffffffffffull      // no key: a key has 63 bits
#define MP_NO_LEADER 0x7fffffff

// ---- host: a call's shape ---------------------------------------------------------------------------------------------------------------
// why a call of num_rows rows in num_clouds clouds into at most max_voxels voxels is refused, or NULL.  An entry without one of the
// three passes a value that is in range (0 rows, 0 clouds, 1 voxel); the size queries answer 0 exactly where an entry refuses
static inline const char* mp_shape_refusal(long long num_rows, int num_clouds, long long max_voxels) {
    if (!(num_rows >= 0 && num_rows < 2147483648ll)) return "need 0 <= num_rows < 2^31";
    if (!(num_clouds >= 0 && num_clouds <= (1 << 24))) return "need 0 <= num_clouds <= 2^24";
    if (!(max_voxels >= 1 && max_voxels <= (1ll << 28))) return "need 1 <= max_voxels <= 2^28";
    return nullptr;
}
static inline bool mp_supported(long long num_rows, int num_clouds, long long max_voxels) {
    return !mp_shape_refusal(num_rows, num_clouds, max_voxels);
}

static inline unsigned long long mp_cap(long long max_voxels) {
    unsigned long long cap = 1;
    while (cap < 2ull * (unsigned long long)max_voxels + 1) cap <<= 1;
    return cap;
}
static inline long long mp_tiles(long long num_rows) { return (num_rows + MP_TILE - 1) / MP_TILE; }
static inline long long mp_groups(long long num_rows) { return (mp_tiles(num_rows) + MP_GROUP - 1) / MP_GROUP; }

__device__ __forceinline__ int mp_load(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// ---- the rows of a tile -----------------------------------------------------------------------------------------------------------------
// A row's kind: 0 kept (then w holds the lattice coordinates), 1 absent, 2 out of range.  m: the pose's twelve entries, d = fl(t - origin).
__device__ __forceinline__ int mp_row(const double* __restrict__ m, const double* __restrict__ d, double voxel, float xf, float yf, float zf,
                                      long long* w) {
#pragma clang fp contract(off)
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    const double q0 = ((m[0] * x + m[1] * y) + m[2] * z) + d[0];
    const double q1 = ((m[4] * x + m[5] * y) + m[6] * z) + d[1];
    const double q2 = ((m[8] * x + m[9] * y) + m[10] * z) + d[2];
    const double s0 = (q0 / voxel) * 4096.0, s1 = (q1 / voxel) * 4096.0, s2 = (q2 / voxel) * 4096.0;
    if (!(__builtin_isfinite(s0) && __builtin_isfinite(s1) && __builtin_isfinite(s2))) return 1;
    const double f0 = __builtin_floor(s0), f1 = __builtin_floor(s1), f2 = __builtin_floor(s2);
    const double lim = 4294967296.0;
    if (!(f0 >= -lim && f0 < lim && f1 >= -lim && f1 < lim && f2 >= -lim && f2 < lim)) return 2;
    w[0] = (long long)f0, w[1] = (long long)f1, w[2] = (long long)f2;
    return 0;
}

// ---- cells, keys and the table (SLOT: a slot type whose first member is `unsigned long long key`) ------------------------------------------
// the key of the cell (g0, g1, g2), each in [-EPC_MAP_MAX_CELL, EPC_MAP_MAX_CELL): of a row's cell (w >> 12) and of every neighbour cell
// that is looked up
__device__ __forceinline__ unsigned long long mp_key(long long g0, long long g1, long long g2) {
    return ((unsigned long long)(g2 + EPC_MAP_MAX_CELL) << 42) | ((unsigned long long)(g1 + EPC_MAP_MAX_CELL) << 21) |
           (unsigned long long)(g0 + EPC_MAP_MAX_CELL);
}
// the cell of a key
__device__ __forceinline__ void mp_cell(unsigned long long key, long long& g0, long long& g1, long long& g2) {
    g0 = (long long)(key & 0x1fffff) - EPC_MAP_MAX_CELL, g1 = (long long)((key >> 21) & 0x1fffff) - EPC_MAP_MAX_CELL;
    g2 = (long long)((key >> 42) & 0x1fffff) - EPC_MAP_MAX_CELL;
}
__device__ __forceinline__ bool mp_in_range(long long c) { return c >= -EPC_MAP_MAX_CELL && c < EPC_MAP_MAX_CELL; }

// the hash of a key: the finaliser of splitmix64 (the output does not depend on it)
__device__ __forceinline__ unsigned long long mp_hash(unsigned long long k) {
    k ^= k >> 30;
    k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27;
    k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return k;
}

// The slot of `key`, claimed by a 64-bit atomicCAS where the table does not hold it yet (linear probing; *claimed counts the claims), or
// -3: the table overflowed -- a full table holds no empty slot: the count of claimed slots is what ends the walk, and a probe gives up
// every 8th step once it sees more than max_voxels.
template <typename SLOT>
__device__ __forceinline__ int mp_claim(SLOT* __restrict__ table, unsigned long long mask, unsigned long long key, int32_t* claimed,
                                        long long max_voxels) {
    unsigned long long s = mp_hash(key) & mask;
    for (unsigned probes = 0;; ++probes) {
        if ((probes & 7) == 0 && (long long)mp_load(claimed) > max_voxels) return -3;
        unsigned long long* kp = &table[s].key;
        unsigned long long k = __atomic_load_n(kp, __ATOMIC_RELAXED);
        if (k == MP_EMPTY) {
            k = atomicCAS(kp, MP_EMPTY, key);
            if (k == MP_EMPTY) {
                atomicAdd(claimed, 1);
                k = key;
            }
        }
        if (k == key) return (int)s;
        s = (s + 1) & mask;
    }
}

// the slot of `key`, or -1: the walk ends at the key or at an empty slot (the table is at most half full)
template <typename SLOT>
__device__ __forceinline__ long long mp_find(const SLOT* __restrict__ table, unsigned long long mask, unsigned long long key) {
    unsigned long long s = mp_hash(key) & mask;
    for (;;) {
        const unsigned long long k = table[s].key;
        if (k == key) return (long long)s;
        if (k == MP_EMPTY) return -1;
        s = (s + 1) & mask;
    }
}

// ---- the leaders' scan: a voxel's number is the rank of its leader, the first row that reached its slot --------------------------------------
// the call has no map: the offsets were not valid, or more voxels than max_voxels were claimed (row_slot and the table may not be followed)
__device__ __forceinline__ bool mp_no_map(const int32_t* head, long long max_voxels) {
    return head[MP_BAD] != 0 || (long long)head[MP_CLAIMED] > max_voxels;
}

template <typename SLOT>
__device__ __forceinline__ int mp_is_leader(const SLOT* table, const int32_t* row_slot, long long r, long long num_rows, int* slot) {
    if (r >= num_rows) return 0;
    const int s = row_slot[r];
    *slot = s;
    return s >= 0 && table[s].leader == (int)r ? 1 : 0;
}

// level 0 is a count kernel's own block_scan of mp_is_leader over its tile
// level 1, one workgroup of MP_GROUP threads: the tiles' counts of its group to exclusive prefixes, the group's total to group[blockIdx.x]
__device__ __forceinline__ void mp_scan_group(long long tiles, int32_t* __restrict__ tile, int32_t* __restrict__ group, int* part) {
    const long long t = (long long)blockIdx.x * MP_GROUP + threadIdx.x;
    const int v = t < tiles ? tile[t] : 0;
    int total;
    const int excl = block_scan<MP_GROUP / 64, int>(v, part, total);
    if (t < tiles) tile[t] = excl;
    if (threadIdx.x == 0) group[blockIdx.x] = total;
}
// level 2, ONE workgroup of MP_THREADS threads: the groups' totals to exclusive prefixes in chunks of its width with a running carry ->
// the sum of all
__device__ __forceinline__ int mp_scan_top(long long groups, int32_t* __restrict__ group, int* part) {
    int carry = 0;
    for (long long base = 0; base < groups; base += MP_THREADS) {
        const long long g = base + threadIdx.x;
        const int v = g < groups ? group[g] : 0;
        int total;
        const int excl = carry + block_scan<MP_THREADS / 64, int>(v, part, total);
        if (g < groups) group[g] = excl;
        carry += total;
    }
    return carry;
}
// what a one-shot entry's level 2 writes besides: V and the three row counts, from the head
__device__ __forceinline__ void mp_top(const int32_t* head, long long groups, int32_t* group, long long max_voxels, int32_t* num_out,
                                       int* part) {
    const bool bad = head[MP_BAD] != 0, none = mp_no_map(head, max_voxels);
    if (!none) mp_scan_top(groups, group, part);
    if (threadIdx.x == 0) {
        num_out[0] = none ? -1 : head[MP_CLAIMED];                          // V: every claimed slot has a leader
        num_out[1] = bad ? 0 : head[MP_KEPT];
        num_out[2] = bad ? 0 : head[MP_KEPT + 1];
        num_out[3] = bad ? 0 : head[MP_KEPT + 2];
    }
}
#endif
