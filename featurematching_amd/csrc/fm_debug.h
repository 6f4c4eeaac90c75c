/*
 * fm_debug.h - diagnostic entry points of libfmatch_hip.so.  NOT part of the drop-in boundary (include/fmatch.h): they
 * launch single kernels of the coarse stage on a workspace a complete call has filled, so that bench.py and the tools/
 * scripts can bracket one kernel with events, and expose the workspace layout to the tests.  A caller of the library
 * never needs them.
 */
#ifndef FM_DEBUG_H_
#define FM_DEBUG_H_

#include "fmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic only: workspace layout of fm_coarse_match (40 values: 10 ints, byte offsets, the screening
 * kernel's split geometry, total; order documented in csrc/api.hip) so tests can inspect
 * intermediate statistics. */
int fm_debug_coarse_layout(int N, int L, int S, int C, int cand_slots, int64_t* out, int n_out);

/* Diagnostic only: launch one kernel of the coarse stage (fm_debug_launch_corr: mode 0 = max pass,
 * 1 = dense sum kernel, 2 = exact screening sweep; fm_debug_launch_screen: the screening kernel k_screen / k_thresh + k_screen_rows) on a
 * workspace filled by a previous fm_coarse_match of the same shapes and inputs / zero the candidate counters
 * and scalars so that the sum kernels can run again; used by bench.py to bracket the dominant kernels with
 * events on their own stream.  Modes 1 / 2 and fm_debug_launch_prep_f16 need a full-size workspace
 * (fm_coarse_workspace_bytes). */
int fm_debug_launch_corr(void* workspace, int N, int L, int S, int C, int cand_slots,
                         float temperature, float thr, int mode, void* stream);
int fm_debug_launch_screen(void* workspace, const float* feat0, const float* feat1, int N, int L, int S,
                               int C, int cand_slots, float temperature, float thr, void* stream);   /* float32 rows */
int fm_debug_launch_prep(void* workspace, const float* feat0, const float* feat1, int N, int L, int S, int C,
                         int cand_slots, void* stream);      /* k_prep_split alone; clears the per-call counters */
int fm_debug_launch_prep_f16(void* workspace, const float* feat0, const float* feat1, int N, int L, int S, int C,
                             int cand_slots, int force, void* stream);
int fm_debug_reset_counters(void* workspace, int N, int L, int S, int C, int cand_slots, void* stream);
/* FM_MODE_FLAT's two own launches alone: which = 0 k_prep_split with the float16 planes (clears the per-call counters
 * like fm_debug_launch_prep), which = 1 the stabiliser kernel k_stab.  Full-size workspace. */
int fm_debug_launch_flat(void* workspace, const float* feat0, const float* feat1, int N, int L, int S, int C,
                         int cand_slots, float temperature, float thr, int which, void* stream);
/* Test-only, process-global: the unit certificate of the screening (the max pass publishes every 32 x 32 unit's
 * runner-up and the place of its maximum; k_screen_rows resolves the units they certify without sweeping them).
 * mode 0 = the launch plan decides (default), 1 = off, 2 = on for every shape (and k_screen_rows counts the live units
 * it certified); any other value only reads.  Returns the previous mode.  Set it between complete calls only.
 * (The plan takes the certificate on the common path only - not with FM_MODE_DENSE / FM_MODE_FLAT / statistics of every
 * row; fm_debug_launch_corr, which knows no mode, follows the shape's rule alone.) */
int fm_debug_unit_cert(int mode);
/* Byte offsets in the coarse workspace of umax, umax2, upos, thr_r, thr_c, tmin_r, tmin_c and the counter of certified
 * units (int32, zeroed per call), then whether the launch plan of this shape uses the certificate (9 values). */
int fm_debug_unit_cert_layout(int N, int L, int S, int C, int cand_slots, int64_t* out, int n_out);
/* Test-only, process-global: the deferred exact dot products of the screening (k_screen_rows lists an entry whose
 * integer screening product proves it significant for its row and its column with a tagged index and a stand-in value,
 * without gathering the two descriptor rows; k_select forms the exact product of the few it needs).
 * mode 0 = the launch plan decides (default: on the common path, where k_select is the lists' only reader), 1 = off,
 * 2 = as 0, and k_screen_rows counts the deferred entries; any other value only reads.  Returns the previous mode.  Set
 * it between complete calls only.  fm_debug_launch_screen, which knows no mode, defers unless the switch is 1. */
int fm_debug_defer_exact(int mode);
/* Byte offset in the coarse workspace of the counter of deferred entries (int32, zeroed per call), the tag bit of a list
 * index, and whether a common-path call of this shape defers under the present switch (3 values). */
int fm_debug_defer_exact_layout(int N, int L, int S, int C, int cand_slots, int64_t* out, int n_out);
/* The five-point solver of fm_estimate_pose (k_pose_solve) alone, on the caller's samples: q0, q1 [dev] float64 [S, 5, 2]
 * normalised coordinates -> E_out [dev] float64 [S, 10, 9] (the first count_out[s] of a sample's ten slots are written:
 * unit Frobenius norm, ascending z) and count_out [dev] int32 [S].  FM_E_NULL, FM_E_SHAPE (S <= 0), a hipError_t. */
int fm_debug_pose_solve(const double* q0, const double* q1, int S, double* E_out, int32_t* count_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FM_DEBUG_H_ */
