/* epcnet_scans.h -- preparation of raw scans in front of the down-sampler: the third header of libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others from epcnet.h and epcnet_poses.h.  The entries carry the prefix epcnet_: epcnet.h stays the complete list of the
 * library's epc_ symbols.
 */
#ifndef EPCNET_SCANS_H
#define EPCNET_SCANS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------ */
/* Ground removal: "the largest near-horizontal plane of the scan, and everything at or below it, goes"     */
/* -- csrc/ground.hip; numpy restatement: tests/ground_ref.py                                               */
/* ------------------------------------------------------------------------------------------------------ */
/* A deterministic plane RANSAC per scan.  Everything is float32 and every operation is rounded once (no FMA, no sqrt, no division),
 * written fl(.) below, so numpy's float32 decides every row alike: the outputs are the same bits on every run and equal to the
 * restatement's.  The frame is the sensor's with z up.  It removes one plane and what lies below it; it is not a terrain model.
 *
 * points (num_rows, 3) float32: the packed rows of all scans; offsets (num_clouds + 1) int32 in DEVICE memory, read when the kernels
 * run: scan b is the rows [offsets[b], offsets[b + 1]).  The offsets are valid iff 0 <= offsets[0], they are non-decreasing and
 * offsets[num_clouds] <= num_rows.  If they are not, EVERY scan fails: status EPC_STATUS_NO_GROUND, info 0 0 0 0, plane NaN, all rows
 * copied unchanged.  With valid offsets a scan of more than 2^20 rows fails alone in the same way.  Rows inside no scan are copied
 * unchanged.
 *
 * The hash:  mix(x) of epcnet_poses.h;  s = mix((uint32)seed);  s = mix(s ^ (uint32)(seed >> 32));  s_h = mix(s ^ h)  for hypothesis
 * h in [0, hypotheses).  Neither the scan's index nor its place in the batch enters: a scan gives the same bits wherever it stands.
 *
 * Vertex j (0, 1, 2) of hypothesis h in a scan of M rows, with K = draws: the candidate rows are
 *     r_k = (uint64(mix(s_h ^ (K * j + k))) * M) >> 32       for k = 0 .. K - 1;
 * of the candidates whose three coordinates are finite the one with the smallest z is the vertex, ties go to the smaller k; if none is
 * finite the hypothesis is invalid.  K = 1 is plain uniform RANSAC; ground is what lies lowest, so K = 8 (the default of
 * ops.remove_ground) finds a ground of a few per cent of the rows where K = 1 does not.
 *
 * The plane of h from its vertices p0, p1, p2:  u = p1 - p0,  v = p2 - p0  per component;
 *     n   = ( fl(fl(u_y v_z) - fl(u_z v_y)),  fl(fl(u_z v_x) - fl(u_x v_z)),  fl(fl(u_x v_y) - fl(u_y v_x)) )
 *     nn  = fl(fl(fl(n_x n_x) + fl(n_y n_y)) + fl(n_z n_z));     if n_z < 0, n is negated (exact);
 *     d0  = fl(fl(fl(n_x x0) + fl(n_y y0)) + fl(n_z z0))
 * h is valid iff its vertices are and  nn >= 1e-12f  (so that flushing a subnormal changes no decision),  nn <= 3e38f,
 * fl(n_z n_z) >= fl(cos2_tilt * nn)  and  d0 <= fl(max_z * n_z)  (max_z = +Inf: no limit; the plane's height at the sensor's axis).
 *     thr = fl(fl(t t) * nn)      with t = threshold
 *     e(row) = fl(fl(fl(fl(n_x x) + fl(n_y y)) + fl(n_z z)) - d0)
 * The score of a valid h is the number of the scan's finite rows (three finite coordinates) with fl(e e) <= thr: an integer count, summed
 * with integer arithmetic only.  The best h has the largest score, ties go to the smaller h.  It is accepted iff score >= 3 and
 * (float)score >= fl(min_share * (float)finite_rows).  Without an accepted plane the scan gets EPC_STATUS_NO_GROUND, a NaN plane and its
 * rows copied unchanged: a missing plane is reported, nothing is removed on a guess.
 *
 * Removal: a finite row goes iff e < 0 or fl(e e) <= thr; its three words become 0x7fc00000, which epc_grid_downsample drops.  Every
 * other row keeps its bits, non-finite rows included.  points_out (num_rows, 3) may be points itself.
 *
 * plane (num_clouds, 4) float32: n_x, n_y, n_z, d0 of the accepted hypothesis, else four NaN.  info (num_clouds, 4) int32, may be NULL:
 * finite rows, valid hypotheses, the best h (-1 if none is valid), its score (0 if none is valid).  status (num_clouds int32):
 * OVERWRITTEN per scan with 0 or EPC_STATUS_NO_GROUND.
 *
 * Four launches on `stream` with grids sized from num_rows, num_clouds and hypotheses alone, the counters zeroed by the call itself:
 * capturable in a graph and replayable on other offsets.  EPC_EINVAL, with nothing launched and nothing written, unless
 * 0 <= num_rows, 0 <= num_clouds <= 65535, hypotheses is a multiple of 64 in [64, 1024], draws is in [1, 16], threshold is finite and
 * > 0, cos2_tilt is in (0, 1], max_z is not NaN, min_share is in [0, 1], and workspace is 16-byte aligned; EPC_ENOMEM for a workspace
 * shorter than epcnet_ground_workspace_bytes(num_clouds, hypotheses, num_rows), which launches nothing and returns 0 for
 * unsupported arguments. */
#define EPC_STATUS_NO_GROUND 8 /* epcnet_ground_remove: no accepted ground plane; the scan's rows are returned unchanged   */
#define EPC_GROUND_MAX_ROWS 1048576
size_t epcnet_ground_workspace_bytes(int num_clouds, int hypotheses, long long num_rows);
int epcnet_ground_remove(const float* points, const int32_t* offsets, int num_rows, int num_clouds, int hypotheses, int draws,
                         float threshold, float cos2_tilt, float max_z, float min_share, long long seed, float* points_out, float* plane,
                         int32_t* info, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_SCANS_H */
