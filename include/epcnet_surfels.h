/* epcnet_surfels.h -- the voxel map with a surfel per voxel (centroid, normal, eigenvalues of the pooled covariance): the eleventh header
 * of libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others (one row of its table of headers).  The entries carry the prefix epcnet_: epcnet.h stays the complete list of the
 * library's epc_ symbols.
 */
#ifndef EPCNET_SURFELS_H
#define EPCNET_SURFELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------ */
/* Map surfels: "the map of epcnet_map_fuse, and per voxel the local surface: where it is, which way it      */
/* faces, how flat it is" -- csrc/surfel.hip; numpy restatement: tests/surfel_ref.py                         */
/* ------------------------------------------------------------------------------------------------------ */
/* A 0.2 m voxel holds two or three rows: its own rows carry no covariance.  The statistics of voxel j are therefore POOLED over the
 * (2 ring + 1)^3 cells around it, from integer moments that every voxel keeps of its own rows.  The moments and their pooled sums are
 * integers, so they do not depend on the order in which rows or cells arrive; everything behind them is a fixed sequence of FLOAT64
 * operations, each rounded once (no FMA), written fl(.) below: + - * /, the correctly rounded square root, comparisons and selects.
 * The outputs are the same bits on every run and equal to the restatement's.
 *
 * Inputs, limits and refusals are those of epcnet_map_fuse (epcnet_maps.h): points, offsets, num_rows, num_clouds, poses, origin in
 * DEVICE memory, max_voxels; besides
 *   params: EIGHT doubles in HOST memory, read during the call: voxel, min_count, ring, min_support, 0, 0, 0, 0.
 *       ring: an integer value in [0, EPC_SURFEL_MAX_RING]; min_support: an integer value in [3, 2^31).
 *
 * Rows, cells, keys, leaders, numbering: word for word those of epcnet_maps.h -- d_a, q_a, s_a, f_a, ABSENT / OUT OF RANGE / KEPT,
 * w_a = (int64) f_a, the cell g_a = w_a >> 12, the key, a voxel's leader, the voxels numbered j = 0 .. V - 1 by ascending leader,
 * cnt_j, S_j, m_j.  map_points, count and num_out are defined as there and are BIT-EQUAL to what epcnet_map_fuse writes for the same
 * voxel, min_count and max_voxels.
 *
 * Own moments.  Per voxel, over its kept rows, with u_a = (w_a & 4095) >> 4 (a lattice of voxel / 256 inside the cell, 0 .. 255):
 *     n = cnt          A_a = sum of u_a          B_ab = sum of u_a u_b    (a <= b: six sums)
 * all int64.
 *
 * Pool.  For voxel j with cell g, over every cell g + o with o in [-ring, ring]^3: the cell COUNTS iff g_a + o_a lies in
 * [-EPC_MAP_MAX_CELL, EPC_MAP_MAX_CELL) on every axis (a cell outside the range is skipped, never wrapped), it is a voxel, and its
 * cnt >= min_count; the own cell (o = 0) is under the same rule.  With (n', A', B') its moments and e_a = 256 o_a, it adds, in the
 * frame of cell g,
 *     N     += n'
 *     S1_a  += A'_a + n' e_a
 *     S2_ab += B'_ab + e_a A'_b + e_b A'_a + n' e_a e_b
 * in int64.  Bounds: a pooled coordinate u_a + e_a lies in [-512, 767], so |coordinate| <= 768; N <= num_rows < 2^31, hence
 * |S1_a| < 2^31 * 768 < 2^41 and |S2_ab| < 2^31 * 768^2 < 2^51: all three convert to float64 EXACTLY, and N fits int32.
 *
 * Covariance, in units of (voxel / 256)^2:
 *     mu_a = fl(S1_a / N)          C_ab = fl(fl(S2_ab / N) - fl(mu_a * mu_b))    for a <= b, mirrored
 * (the subtraction cancels: with coordinates up to 768 both terms reach 6e5, whose float64 spacing is 1.2e-10 -- C carries an absolute
 * error of a few 1e-10 lattice units squared, so a smallest eigenvalue that is exactly 0 may come out as -1e-10: see the clamp).
 *
 * Eigenvectors by cyclic Jacobi exactly as epcnet_pairs.h writes it, on 3 x 3: A = C, V = I, then EPC_SURFEL_SWEEPS sweeps over the
 * pairs (p, q) = (0,1), (0,2), (1,2); r is the third index.  A pair with a_pq == 0 is skipped; otherwise
 *     theta = (a_qq - a_pp) / (2 * a_pq);  t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta * theta + 1))
 *     c = 1 / sqrt(t * t + 1);  s = t * c;  h = t * a_pq
 *     a_pp -= h;  a_qq += h;  a_pq = a_qp = 0
 *     g = a_rp, f = a_rq;  a_rp = a_pr = c * g - s * f;  a_rq = a_qr = s * g + c * f
 *     for i in 0..2:  g = v_ip, f = v_iq;  v_ip = c * g - s * f;  v_iq = s * g + c * f
 * On the numpy restatement 4 sweeps were the smallest count at which one more sweep moved no bit of the float32 outputs below, checked
 * on the scenes of tests/test_surfel_cpu.py and on 320,000 covariances of lattice point sets (random, near-planar, linear, coincident;
 * tests/test_surfel_cpu.py repeats the check); the constant is that count plus one.
 *
 * Eigenvalues: the three a_kk in ascending order, ties to the lower k: k0 = the k with the smallest a_kk (k = 1, 2 replace the
 * incumbent only when strictly smaller), then the other two in index order, swapped only when the later is strictly smaller.
 * lambda = a_kk < 0 ? +0.0 : a_kk.
 *
 * Normal: v = column k0 of V; nn = sqrt(fl(fl(v_0 v_0 + v_1 v_1) + v_2 v_2)) (each product rounded), n_a = fl(v_a / nn); the whole
 * vector is negated when its component of largest magnitude is negative (k = 1, 2 replace the incumbent only when |n_k| is strictly
 * larger: ties go to the lower axis).  It is NOT oriented towards a viewpoint.
 *
 * Outputs; EVERY word is written on every call.  With s = fl(voxel / 256):
 *   map_points (max_voxels, 3) float32, count (max_voxels) int32, num_out (4) int32: as epcnet_map_fuse.
 *   support (max_voxels) int32: N_j for every j < V (whatever min_count and min_support), 0 behind.
 *   A surfel is VALID iff cnt_j >= min_count and N_j >= min_support.  For a valid one
 *   centroid (max_voxels, 3) float32: (float) fl(fl((double)(256 g_a) + mu_a) * s), metres relative to origin.  u_a is a floor: the
 *       centroid lies below the mean of the rows by less than voxel / 256 on every axis (0.8 mm at 0.2 m).
 *   eigen (max_voxels, 3) float32: (float) fl(fl(lambda_k * s) * s), ascending, in m^2.
 *   normal (max_voxels, 3) float32: (float) n_a, in the map's axes.
 *   Otherwise, and for j >= V, the nine words are 0x7fc00000.
 * Overflow (V > max_voxels) and invalid offsets: num_out as epcnet_map_fuse reports them, every float word 0x7fc00000, every count and
 * support 0.
 *
 * Seven launches and no memset on `stream`, sized from num_rows and max_voxels alone; capturable and replayable on other points,
 * offsets, poses and origin (params are part of the capture).  Integer atomics only.  The workspace holds an open-addressing table
 * (the smallest power of two >= 2 max_voxels + 1 slots of 128 bytes), 4 bytes per row and 4 bytes per 256 rows.  EPC_EINVAL, with
 * nothing launched and nothing written, under the rules of epcnet_map_fuse, and unless ring and min_support are as above and the four
 * reserved doubles are 0; EPC_ENOMEM for a workspace shorter than epcnet_map_surfels_workspace_bytes(num_rows, num_clouds,
 * max_voxels), which launches nothing and returns 0 for unsupported arguments.
 *
 * Not covered: normals oriented towards a viewpoint.  Point-to-plane registration against the surfels is epcnet_localize.h; the same map
 * kept across calls and grown by the rows added is epcnet_growmap.h. */
#define EPC_SURFEL_PARAMS 8
#define EPC_SURFEL_MAX_RING 2
#define EPC_SURFEL_SWEEPS 5
size_t epcnet_map_surfels_workspace_bytes(long long num_rows, int num_clouds, long long max_voxels);
int epcnet_map_surfels(const float* points, const int32_t* offsets, long long num_rows, int num_clouds, const double* poses,
                       const double* origin, const double* params, long long max_voxels, float* map_points, int32_t* count,
                       float* centroid, float* normal, float* eigen, int32_t* support, int32_t* num_out,
                       void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_SURFELS_H */
