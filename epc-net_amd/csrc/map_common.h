// What the two voxel-map files share (map.hip: epcnet_map_fuse; surfel.hip: epcnet_map_surfels): the definition's row -> lattice step, the
// key of a cell, the hash of the open-addressing table, the tile / group geometry of the leaders' scan and the words of the workspace's
// head.  map.hip and the surfel files keep their own slot, claim loop and scan kernels: they follow the slot's layout (surfel.hip and
// growmap.hip share theirs through surfel_common.h).
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

static inline unsigned long long mp_cap(long long max_voxels) {
    unsigned long long cap = 1;
    while (cap < 2ull * (unsigned long long)max_voxels + 1) cap <<= 1;
    return cap;
}
static inline long long mp_tiles(long long num_rows) { return (num_rows + MP_TILE - 1) / MP_TILE; }
static inline long long mp_groups(long long num_rows) { return (mp_tiles(num_rows) + MP_GROUP - 1) / MP_GROUP; }

__device__ __forceinline__ int mp_load(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

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

// the key of the cell (g0, g1, g2), each in [-EPC_MAP_MAX_CELL, EPC_MAP_MAX_CELL): what surfel.hip forms for a row and for every
// neighbour cell it looks up (map.hip's insert kernel spells the same expression out on w >> 12)
__device__ __forceinline__ unsigned long long mp_key(long long g0, long long g1, long long g2) {
    return ((unsigned long long)(g2 + EPC_MAP_MAX_CELL) << 42) | ((unsigned long long)(g1 + EPC_MAP_MAX_CELL) << 21) |
           (unsigned long long)(g0 + EPC_MAP_MAX_CELL);
}

// the hash of a key: the finaliser of splitmix64 (the output does not depend on it)
__device__ __forceinline__ unsigned long long mp_hash(unsigned long long k) {
    k ^= k >> 30;
    k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27;
    k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return k;
}
#endif
