/* epcnet_maps.h -- corrected submaps fused into one voxel map, behind the loop closing: the tenth header of libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others (one row of its table of headers).  The entries carry the prefix epcnet_: epcnet.h stays the complete list of the
 * library's epc_ symbols.
 */
#ifndef EPCNET_MAPS_H
#define EPCNET_MAPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------ */
/* A map in one frame: "every kept row of every cloud moved by its cloud's pose, one point per voxel"        */
/* -- csrc/map.hip; numpy restatement: tests/map_ref.py                                                      */
/* ------------------------------------------------------------------------------------------------------ */
/* Every row is moved into the world frame in FLOAT64 with every operation rounded once (no FMA), written fl(.) below, and lands on an
 * INTEGER lattice of voxel / 4096; from there on everything is integer -- the voxel a row falls in, the sums of the rows' positions
 * inside it, the mean -- so no result depends on the order in which the rows arrive: the outputs are the same bits on every run and
 * equal to the restatement's.  Poses are UTM-sized (a northing near 5.7e6 has a float32 spacing of 0.5 m): they stay float64, and the
 * map's coordinates are relative to `origin`, so that they fit float32.
 *
 * Inputs, in DEVICE memory and read when the kernels run unless marked:
 *   points (num_rows, 3) float32, offsets (num_clouds + 1) int32: packed ragged clouds, cloud c is the rows [offsets[c], offsets[c + 1]).
 *       Valid by the rule of epcnet_scans.h: 0 <= offsets[0], non-decreasing, offsets[num_clouds] <= num_rows.  These are the
 *       sub_points, sub_offsets of epcnet_submap_build, with or without epcnet_ground_remove applied: NaN rows are absent.  A row in
 *       front of offsets[0] or at and behind offsets[num_clouds] belongs to no cloud: it is no row of the map and is not counted.
 *   poses (num_clouds, 12) float64: row-major [R | t], cloud to world: R[a][b] at 4a + b, t[a] at 4a + 3 -- the poses_out of
 *       epcnet_trajectory_relax, or the sub_pose of epcnet_submap_build.
 *   origin (3) float64: the world point the map's coordinates are relative to.  Device memory: a captured graph replays on another
 *       trajectory.
 *   params: EIGHT doubles in HOST memory, read during the call (the grammar has no double scalar here): voxel, min_count, 0, 0, 0, 0,
 *       0, 0.
 *   max_voxels: the caller's capacity, in rows of map_points and words of count.
 *
 * Per row (x, y, z) of cloud c, widened to float64 (exact), with R, t the cloud's pose:
 *     d_a = fl(t_a - origin_a)
 *     q_a = fl(fl(fl(fl(R[a][0] x) + fl(R[a][1] y)) + fl(R[a][2] z)) + d_a)                              a = 0, 1, 2
 *     s_a = fl(fl(q_a / voxel) * 4096)          (IEEE division; the product is exact or overflows)
 *     f_a = floor(s_a)
 * The row is ABSENT iff some s_a is not finite (a NaN row, a NaN pose, a NaN origin).  Otherwise it is OUT OF RANGE iff some f_a lies
 * outside [-2^32, 2^32), compared in float64 before any conversion.  Otherwise it is KEPT: w_a = (int64) f_a, its cell is
 * g_a = w_a >> 12 (arithmetic shift: floor(q_a / voxel), in [-EPC_MAP_MAX_CELL, EPC_MAP_MAX_CELL)), its position inside the cell is
 * w_a & 4095, and its key is ((g_2 + 2^20) << 42) | ((g_1 + 2^20) << 21) | (g_0 + 2^20).
 *
 * Per voxel.  A voxel is a key that at least one kept row has.  Its LEADER is the smallest source row index with that key; the voxels
 * are numbered j = 0 .. V - 1 by ascending leader (deterministic, and no sort).  cnt_j is its number of kept rows, S_j[a] the integer
 * sum of w_a & 4095 over them (int64: free of summation order), m_j[a] = S_j[a] // cnt_j by integer floor division.
 *
 * Outputs; EVERY word is written on every call:
 *   map_points (max_voxels, 3) float32: for j < V and cnt_j >= min_count, row j is
 *           (float) fl((double)(g_a * 4096 + m_j[a]) * fl(voxel / 4096))                                 a = 0, 1, 2
 *       in metres relative to origin (ONE rounding to float32, IEEE to nearest even: numpy's astype); for j < V and cnt_j < min_count
 *       three words 0x7fc00000 -- the rule of a cropped row of epcnet_submap_build: a voxel that a passing car hit once goes, nothing
 *       is compacted --; for j >= V three words 0x7fc00000.  epc_grid_downsample and epcnet_pair_register treat such rows as absent,
 *       so the map feeds them with no host read (e.g. registering a new submap against the map).
 *   count (max_voxels) int32: cnt_j, whatever min_count; 0 for j >= V.
 *   num_out (4) int32: V, rows kept, rows absent, rows out of range.
 * Overflow: if V > max_voxels then num_out[0] = -1, every row of map_points is NaN words and every count is 0; the three row counts
 * are reported as usual.  Whole-call failure, decided on the device: if the offsets are not valid, num_out = -1, 0, 0, 0 with the same
 * NaN / 0 outputs.
 *
 * Seven launches and no memset on `stream` (the first clears the workspace's head), sized from num_rows and max_voxels alone; the call
 * zeroes what it counts in: capturable in a graph and replayable on other points, offsets, poses and origin (params are read at the
 * call: they are part of the capture).  Integer atomics only.  The workspace holds an open-addressing table whose size depends on
 * max_voxels alone (the smallest power of two >= 2 max_voxels + 1 slots of 40 bytes), 4 bytes per row and 4 bytes per 256 rows.
 * EPC_EINVAL, with nothing launched and nothing written, unless 0 <= num_rows < 2^31, 0 <= num_clouds <= 2^24, 1 <= max_voxels <= 2^28,
 * voxel is finite and lies in [2^-20, 2^20], min_count is an integer value in [1, 2^31), the six reserved doubles are 0, every pointer
 * is non-NULL and the workspace is 16-byte aligned; EPC_ENOMEM for a workspace shorter than
 * epcnet_map_fuse_workspace_bytes(num_rows, num_clouds, max_voxels), which launches nothing and returns 0 for unsupported arguments. */
#define EPC_MAP_PARAMS 8
#define EPC_MAP_MAX_CELL 1048576 /* cells per axis on either side of the origin: 2^20 */
size_t epcnet_map_fuse_workspace_bytes(long long num_rows, int num_clouds, long long max_voxels);
int epcnet_map_fuse(const float* points, const int32_t* offsets, long long num_rows, int num_clouds, const double* poses,
                    const double* origin, const double* params, long long max_voxels, float* map_points, int32_t* count,
                    int32_t* num_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_MAPS_H */
