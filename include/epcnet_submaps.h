/* epcnet_submaps.h -- travel-length submaps from posed scans, in front of the ground removal and the down-sampler: the fourth header of
 * libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others from epcnet.h, epcnet_poses.h and epcnet_scans.h.  The entries carry the prefix epcnet_: epcnet.h stays the
 * complete list of the library's epc_ symbols.
 */
#ifndef EPCNET_SUBMAPS_H
#define EPCNET_SUBMAPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------ */
/* Submaps: "every return gathered along a fixed length of travel, in the frame of the scan at its middle"   */
/* -- csrc/submap.hip; numpy restatement: tests/submap_ref.py                                                */
/* ------------------------------------------------------------------------------------------------------ */
/* The trajectory is cut by travelled distance, every scan of a submap is moved into the submap's frame and cropped.  Everything is
 * FLOAT64 with every operation rounded once (no FMA, no sqrt, no division), written fl(.) below, then ONE rounding to float32
 * (IEEE, to nearest even: numpy's astype), so numpy's float64 decides every row alike: the outputs are the same bits on every run
 * and equal to the restatement's.  Poses are UTM-sized (a northing near 5.7e6 has a float32 spacing of 0.5 m): they stay float64.
 *
 * Inputs, in DEVICE memory and read when the kernels run unless marked:
 *   points (num_rows, 3) float32, offsets (num_scans + 1) int32: the packed scans in the order they were taken; scan i is the rows
 *       [offsets[i], offsets[i + 1]).  Valid by the rule of epcnet_scans.h: 0 <= offsets[0], non-decreasing, offsets[num_scans] <=
 *       num_rows.
 *   poses (num_scans, 12) float64: row-major [R | t], sensor to world: R[a][b] at 4a + b, t[a] at 4a + 3.
 *   along (num_scans) float64: the travelled distance at each scan, non-decreasing.  (The kernels take no square root: the caller,
 *       or ops.build_submaps, sums the step lengths.  That keeps the segmentation exact and order-free.)
 *   params: EIGHT doubles in HOST memory, read during the call (as epcnet_poses.h passes a radius: the grammar has no double
 *       scalar): length, spacing, min_range, max_range, z_min, z_max, 0, 0.
 *   max_submaps, out_rows: the caller's capacities, in slots and in rows of points_out.
 *
 * Segmentation.  h = fl(length * 0.5).  For slot k in [0, max_submaps]:
 *     c_k = fl(fl(along[0] + h) + fl((double)k * spacing)),   s_k = fl(c_k - h),   e_k = fl(c_k + h).
 * Slot k is a SUBMAP iff e_k <= along[num_scans - 1]; e_k does not decrease with k, so the submaps are a prefix of the slots.  Its
 * scans are [lo_k, hi_k): lo_k the first i with along[i] >= s_k, hi_k the first i with along[i] >= e_k (num_scans if none).  Its frame
 * is that of scan ref_k, the first i with along[i] >= c_k: it exists (c_k <= e_k <= along[num_scans - 1]); it need not lie in
 * [lo_k, hi_k) when `along` jumps, and a submap may hold no scan at all: it then has zero rows and status 0 (the down-sampler
 * reports it as EPC_STATUS_NO_GRID).  The three indices are lower bounds in a sorted array.  spacing < length overlaps the submaps (a
 * scan then belongs to several), spacing == length abuts them, spacing > length leaves gaps.
 *
 * Layout.  rows_k = offsets[hi_k] - offsets[lo_k] for a submap; rows_k counts as 0 for a slot that is no submap and for a submap of
 * more than EPC_SUBMAP_MAX_ROWS rows (the limit of epc_grid_downsample and epcnet_ground_remove), which gets EPC_STATUS_NO_ROOM.
 * P is the exclusive prefix sum of rows_k over the slots, in integers.  Submap k FITS iff P[k + 1] <= out_rows; P is monotone, so the
 * submaps that do not fit are the last ones.  With k_fit the number of submaps that fit,
 *     sub_offsets[k] = min(P[k], P[k_fit])      for k in [0, max_submaps]        (int32)
 * so a submap that does not fit has zero rows; it gets EPC_STATUS_NO_ROOM.  A slot that is no submap has zero rows and
 * EPC_STATUS_NO_SUBMAP.  Row j of submap k in points_out (out_rows, 3) is source row offsets[lo_k] + j: the order of the scans and of
 * their rows is kept.  Rows of points_out at and beyond sub_offsets[max_submaps] keep whatever they held.
 *
 * Transform.  For scan i of submap k, with r = ref_k, Ri, ti and Rr, tr the two poses and d = fl(ti - tr) per component:
 *     M[a][b] = fl(fl(fl(Rr[0][a] Ri[0][b]) + fl(Rr[1][a] Ri[1][b])) + fl(Rr[2][a] Ri[2][b]))
 *     u[a]    = fl(fl(fl(Rr[0][a] d_0) + fl(Rr[1][a] d_1)) + fl(Rr[2][a] d_2))
 * and for a row (x, y, z) of the scan, widened to float64 (exact):
 *     q_a = fl(fl(fl(fl(M[a][0] x) + fl(M[a][1] y)) + fl(M[a][2] z)) + u[a])                       a = 0, 1, 2
 *     rr  = fl(fl(fl(x x) + fl(y y)) + fl(z z))
 * The row is KEPT iff  rr >= fl(min_range min_range)  (the sensor-frame range: returns from the vehicle itself),
 * fl(fl(q_0 q_0) + fl(q_1 q_1)) <= fl(max_range max_range),  and  z_min <= q_2 <= z_max.  Every comparison is false for a NaN, so a
 * non-finite row or pose drops the row without a special case.  A kept row is written as (float)q_0, (float)q_1, (float)q_2; every
 * other row of the submap as three words 0x7fc00000, which epc_grid_downsample and epcnet_ground_remove treat as absent.  Nothing is
 * compacted: the rule of the ground removal, and every launch's size stays known on the host.
 *
 * Other outputs.  num_out (2) int32: the number of submaps among the slots [0, max_submaps), and 1 if slot max_submaps would have been
 * a submap too (the trajectory holds more submaps than slots), else 0.  sub_pose (max_submaps, 12) float64: a copy of pose ref_k, NaN
 * for a slot that is no submap; its columns 3 and 7 are the (x, y) the entries of epcnet_poses.h take.  sub_info (max_submaps, 4) int32,
 * may be NULL: lo_k, hi_k, ref_k, rows_k (rows_k as counted above: 0 above the row limit, and NOT reduced when the submap does not
 * fit: it says how many rows it needs); -1 -1 -1 0 for a slot that is no submap.  status (max_submaps) int32: OVERWRITTEN per slot with
 * 0, EPC_STATUS_NO_SUBMAP or EPC_STATUS_NO_ROOM.
 *
 * Whole-call failures, decided on the device: if the offsets are not valid, `along` holds a non-finite value or decreases somewhere,
 * or num_scans == 0, then EVERY slot is no submap: EPC_STATUS_NO_SUBMAP, NaN pose, info -1 -1 -1 0, num_out 0 0, every sub_offsets 0,
 * no row of points_out written.  A stationary trajectory (a constant `along`) is valid and has no submap.
 *
 * Five launches and no memset on `stream` (the first clears the workspace's 16-byte head), sized from num_scans, max_submaps and out_rows alone; the call zeroes what it
 * counts in: capturable in a graph and replayable on other points, offsets, poses and along (params are read at the call: they are
 * part of the capture).  Integer atomics only.  EPC_EINVAL, with nothing launched and nothing written, unless 0 <= num_rows,
 * 0 <= num_scans <= 2^24, 1 <= max_submaps <= 65535, 0 <= out_rows < 2^31, length and spacing are finite and > 0, 0 <= min_range,
 * 0 < max_range and it is finite, z_min and z_max are not NaN (-Inf, +Inf: no limit), the two reserved doubles are 0, every pointer
 * but sub_info is non-NULL and the workspace is 16-byte aligned; EPC_ENOMEM for a workspace shorter than
 * epcnet_submap_workspace_bytes(num_scans, max_submaps, num_rows, out_rows), which launches nothing and returns 0 for unsupported
 * arguments. */
#define EPC_STATUS_NO_SUBMAP 16 /* epcnet_submap_build: the slot is no submap (the trajectory ended, or the whole call failed)       */
#define EPC_STATUS_NO_ROOM 32   /* epcnet_submap_build: the submap has more than 2^20 rows, or does not fit out_rows: zero rows     */
#define EPC_SUBMAP_MAX_ROWS 1048576
#define EPC_SUBMAP_PARAMS 8
size_t epcnet_submap_workspace_bytes(int num_scans, int max_submaps, long long num_rows, long long out_rows);
int epcnet_submap_build(const float* points, const int32_t* offsets, long long num_rows, int num_scans, const double* poses,
                        const double* along, const double* params, int max_submaps, long long out_rows, float* points_out,
                        int32_t* sub_offsets, int32_t* num_out, double* sub_pose, int32_t* sub_info, int32_t* status, void* workspace,
                        size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_SUBMAPS_H */
