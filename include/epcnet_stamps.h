/* epcnet_stamps.h -- timestamped scans in front of the submap build: odometry interpolated at each scan's stamp and each sweep
 * de-skewed into the frame of that stamp: the fifth header of libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others from epcnet.h, epcnet_poses.h, epcnet_scans.h and epcnet_submaps.h.  The entries carry the prefix epcnet_:
 * epcnet.h stays the complete list of the library's epc_ symbols.
 */
#ifndef EPCNET_STAMPS_H
#define EPCNET_STAMPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------ */
/* Stamps: "the pose at every scan's time, and every return moved to where the sensor stood at that time"    */
/* -- csrc/stamps.hip; numpy restatement: tests/stamps_ref.py                                                */
/* ------------------------------------------------------------------------------------------------------ */
/* Odometry arrives on its own clock (50 - 200 Hz), scans on another, and a spinning sensor's sweep lasts about 0.1 s, in which the
 * vehicle moves.  The two entries interpolate the odometry at integer times and express every row of a sweep in the sensor frame of
 * the sweep's own stamp.  Times are INTEGER nanoseconds; everything else is FLOAT64 with every operation rounded once (no FMA), written
 * fl(.) below, then ONE rounding to float32 (IEEE, to nearest even: numpy's astype), so numpy's int64 and float64 decide every value
 * alike: the outputs are the same bits on every run and equal to the restatement's.  The definition takes no square root and no
 * transcendental function, and one float64 division per pose (two behind a row: its own pose's and its scan's).  Why a division and
 * no square root: compiled for gfx950 a float64 `/` lowers to the IEEE sequence v_div_scale / v_div_fmas / v_div_fixup, which is
 * correctly rounded, so numpy's `/` gives the same bits; sqrt(double) lowers to v_rsq_f64 and a refinement, whose last bit this
 * definition should not rest on.  That is why the
 * quaternion is never normalised: the rotation matrix is built from the unnormalised quaternion q as I + (2 / |q|^2) (...), which is
 * orthonormal up to rounding for any q != 0.
 *
 * Inputs, in DEVICE memory and read when the kernels run:
 *   points (num_rows, 3) float32, offsets (num_scans + 1) int32: the packed scans; scan i is the rows [offsets[i], offsets[i + 1]).
 *       Valid by the rule of epcnet_scans.h: 0 <= offsets[0], non-decreasing, offsets[num_scans] <= num_rows.
 *   scan_time (num_scans) int64 ns: the instant whose sensor frame scan i is expressed in after de-skewing; typically the sweep's start.
 *   point_dt (num_rows) int32 ns: each row's offset from its scan's time; negative values are allowed (sensors that stamp the sweep's
 *       end).  May be NULL: then nothing is de-skewed, points_out may be NULL too and is not touched, and only scan_pose and status
 *       are produced (the 2-D line scanner's case).
 *   pose_time (num_poses) int64 ns, strictly increasing.
 *   pose (num_poses, 7) float64: tx ty tz qw qx qy qz, sensor to world; the quaternion approximately unit (see above).
 *   max_gap_ns: 1 <= max_gap_ns < 2^31.  A bracket longer than that is an odometry drop-out and is not interpolated across.
 *
 * The pose at an integer time tau.
 *     j   = min(#{k : pose_time[k] <= tau} - 1, num_poses - 2)                     (-1 when tau lies before pose_time[0])
 *     num = tau - pose_time[j],   den = pose_time[j + 1] - pose_time[j]             (int64)
 * The bracket is VALID iff j >= 0, 0 <= num <= den and den <= max_gap_ns: nothing is extrapolated, tau == pose_time[num_poses - 1] is
 * the end of the last bracket.  Then, with (t0, q0) = pose[j] and (t1, q1) = pose[j + 1]:
 *     fi = floor(num * 2^32 / den)          in unsigned 64-bit integers (num < 2^31: the product fits)
 *     f  = (double)fi * 2^-32,   g = 1 - f                                          (both exact)
 * (no float division decides the fraction; its quantisation is 2^-32 of a bracket: 7e-11 m at 30 m/s and 10 ms)
 *     t_a = fl(t0_a + fl(f * fl(t1_a - t0_a)))                                      a = 0, 1, 2
 * Rotation, normalised linear interpolation on the shorter arc (it follows slerp's great arc; only the parameterisation differs, by
 * at most 0.0041 W^3 rad for a bracket angle W up to 1 rad):
 *     d     = fl(fl(fl(fl(w0 w1) + fl(x0 x1)) + fl(y0 y1)) + fl(z0 z1))
 *     sigma = d < 0 ? -1 : 1                                                        (a NaN d: 1)
 *     c     = fl(fl(g * c0) + fl(f * (sigma c1)))                                   for the four components c = w, x, y, z
 *     n     = fl(fl(fl(fl(w w) + fl(x x)) + fl(y y)) + fl(z z))
 *     s     = fl(2 / n)
 *     R00 = fl(1 - fl(s * fl(fl(y y) + fl(z z))))   R01 = fl(s * fl(fl(x y) - fl(w z)))       R02 = fl(s * fl(fl(x z) + fl(w y)))
 *     R10 = fl(s * fl(fl(x y) + fl(w z)))           R11 = fl(1 - fl(s * fl(fl(x x) + fl(z z))))   R12 = fl(s * fl(fl(y z) - fl(w x)))
 *     R20 = fl(s * fl(fl(x z) - fl(w y)))           R21 = fl(s * fl(fl(y z) + fl(w x)))       R22 = fl(1 - fl(s * fl(fl(x x) + fl(y y))))
 * The pose is VALID iff the bracket is valid, n is finite and > 0, and t_0, t_1, t_2 are finite.  It is written row-major as
 * [R | t] -- R[a][b] at 4a + b, t[a] at 4a + 3, the layout epcnet_submap_build takes --; an invalid pose is twelve words
 * 0x7ff8000000000000.  At a knot (num == 0) f is 0 and the translation is the knot's exactly.
 *
 * epcnet_pose_interp.  pose_out (num_queries, 12) float64: the pose at query_time[i]; status (num_queries) int32: OVERWRITTEN with 0 or
 * EPC_STATUS_NO_POSE.  num_queries may be 0 (nothing is launched).  It has no workspace: between its launches status[0] carries the
 * check's verdict (four launches: status[0] cleared, the check, the queries behind the first, the first query).
 *
 * epcnet_scan_deskew.  scan_pose (num_scans, 12) float64: the pose (Rs, ts) at scan_time[i]; status (num_scans) int32: OVERWRITTEN with
 * 0 or EPC_STATUS_NO_POSE.  With point_dt given, row r = (x, y, z) of scan i, widened to float64 (exact), takes the pose (Rp, tp) at
 * scan_time[i] + point_dt[r] (int64):
 *     v_a = fl(fl(fl(Rp[a][0] x) + fl(Rp[a][1] y)) + fl(Rp[a][2] z))
 *     w_a = fl(v_a + fl(tp_a - ts_a))                        (the translations are UTM-sized: they are subtracted first)
 *     q_a = fl(fl(fl(Rs[0][a] w_0) + fl(Rs[1][a] w_1)) + fl(Rs[2][a] w_2))
 * The row is KEPT iff its scan's pose is valid, its own pose is valid and its three input words are finite, and is then written to
 * points_out (num_rows, 3) as (float)q_0, (float)q_1, (float)q_2; every other row of a scan becomes three words 0x7fc00000, which
 * epcnet_submap_build, epcnet_ground_remove and epc_grid_downsample treat as absent.  A scan whose own pose is valid and at least one of
 * whose rows has an invalid pose gets EPC_STATUS_PART_POSE ORed into its status (an integer atomicOr, the only atomic).  Nothing is
 * compacted: `offsets` stays valid for points_out.  Rows outside [offsets[0], offsets[num_scans]) keep whatever they held.
 * points_out == points is refused.
 *
 * Whole-call failures, decided on the device: if the offsets are not valid (epcnet_scan_deskew) or pose_time is not strictly increasing,
 * then EVERY status is EPC_STATUS_NO_POSE, every pose written is twelve NaN words and no row of points_out is written.  (num_poses < 2
 * is refused with EPC_EINVAL before anything is launched.)
 *
 * epcnet_scan_deskew: three launches, four with point_dt, and no memset on `stream`, sized from num_scans, num_poses and
 * num_rows alone; the call zeroes what it counts in: capturable in a graph and replayable on other points, offsets, times and poses.
 * EPC_EINVAL, with nothing launched and nothing written, unless 0 <= num_scans <= 2^24 (0 <= num_queries <= 2^24),
 * 2 <= num_poses <= 2^24, 0 <= num_rows < 2^31, 1 <= max_gap_ns < 2^31, every pointer is non-NULL -- but point_dt, and points_out when
 * point_dt is NULL --, points_out != points and the workspace is 16-byte aligned; EPC_ENOMEM for a workspace shorter than
 * epcnet_deskew_workspace_bytes(num_scans, num_poses, num_rows), which launches nothing and returns 0 for unsupported arguments. */
#define EPC_STATUS_NO_POSE 64    /* the scan's (query's) time has no valid bracket, or the whole call failed: NaN pose, NaN rows */
#define EPC_STATUS_PART_POSE 128 /* some rows of the scan had no valid bracket at their own time and became NaN rows           */
size_t epcnet_deskew_workspace_bytes(int num_scans, int num_poses, long long num_rows);
int epcnet_pose_interp(const long long* pose_time, const double* pose, int num_poses, const long long* query_time, int num_queries,
                       long long max_gap_ns, double* pose_out, int32_t* status, void* stream);
int epcnet_scan_deskew(const float* points, const int32_t* offsets, long long num_rows, int num_scans, const int32_t* point_dt,
                       const long long* scan_time, const long long* pose_time, const double* pose, int num_poses, long long max_gap_ns,
                       float* points_out, double* scan_pose, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_STAMPS_H */
