/*
 * fmatch.h - C ABI of libfmatch_hip.so: the MI355X (gfx950) coarse-to-fine matching
 * hot path.  This is the drop-in boundary for the three stage modules the reference
 * calls from network/net.py:75,78,83 (paths relative to the reference repository):
 *
 *   fm_coarse_match    <- CoarseMatching.forward + get_coarse_match
 *                         network/utils/coarse_matching_new.py:43-143
 *   fm_gather_windows  <- FinePreprocess.forward, window crop + select
 *                         network/module/fine_preprocess.py:43-50
 *   fm_fine_match      <- FineMatching.forward
 *                         network/utils/fine_matching_new.py:22-79
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no framework types.  Every pointer
 *     marked [dev] is device memory owned by the caller; the library never
 *     allocates or frees device memory and keeps no global state.
 *   - All work is enqueued on the caller's stream (a hipStream_t passed as void*;
 *     NULL = the default stream); no call synchronises the host except
 *     fm_read_count.  The caller has made the target device current.
 *   - Return value: 0 = FM_OK, < 0 = invalid use (see enum), > 0 = a hipError_t
 *     passed through.  Functions never throw.
 *   - Data-dependent conditions discovered on the device (capacity overflow,
 *     candidate-slot overflow, non-finite / out-of-range descriptors) are
 *     reported through the status word next to the match count (fm_read_count).
 *   - A workspace may hold anything on entry: no call relies on what an earlier call (or nobody) left in it, except where a
 *     function is documented to read a previous call's results (fm_coarse_cell_maps, fm_coarse_softmax_stats, the resume
 *     inside fm_coarse_match_auto, fm_coarse_loss_backward).
 */
#ifndef FMATCH_H_
#define FMATCH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FM_VERSION 100 /* 0.1.0 */

enum fm_status {
  FM_OK = 0,
  FM_E_NULL = -1,        /* a required pointer is NULL */
  FM_E_SHAPE = -2,       /* L != h0c*w0c, S != h1c*w1c, non-positive size ... */
  FM_E_UNSUPPORTED = -3, /* C > 256 or C % 4 != 0, Cf != 64, W not in {5,7}, thr <= 0 ... */
  FM_E_WORKSPACE = -4,   /* workspace too small / misaligned */
  FM_E_CAPACITY = -5,    /* (device status) more matches than `cap`; M_out = required */
  FM_E_CANDIDATES = -6,  /* (device status) a row or column produced more than cand_slots candidates: call again
                            with mode | FM_MODE_EXACT_SCREENING (then with more cand_slots if it persists) */
  FM_E_RANGE = -7,       /* (device status) a descriptor is not finite or has |x| >= 32768, or the similarities are so
                            large (several thousand: |f0||f1| / (C*temperature)) that the int8 screening margin alone,
                            2^60 in the log2 domain, could overflow the float32 exponentials */
  FM_E_DENSE = -8,       /* (device status) a sample's similarity is flat (more significant entries per 32 x 32 unit
                            than the screening kernel resolves: an untrained network, textureless images); its result
                            is incomplete: call again with mode | FM_MODE_DENSE */
  FM_E_INTERNAL = -9,    /* (device status) the assignment kernel's bounded wait for its predecessor workgroups ran
                            out (never observed; the outputs are incomplete): call again */
  FM_E_STEP = -10        /* (device status) the int8 screening step of an image, estimated from a sample of its rows, is
                            too small for some descriptor outside the sample (an outlier several times larger than the
                            rest, or a sample that fell on textureless cells): what it clipped inflates every screening
                            margin.  The inputs are fine: call again with mode | FM_MODE_EXACT_STEP.  (One step per
                            image bounds the dynamic range the screening can serve: descriptors more than ~5x larger
                            than the rest of their image at C = 256, T = 0.1 still end in FM_E_RANGE - the margin of
                            their coarse codes alone would overflow the exponentials.) */
};

/* `mode` bits of fm_coarse_match / fm_coarse_workspace_bytes_mode (0 = the common path: 4 launches) */
#define FM_MODE_EXACT_SCREENING 1 /* two more kernels re-screen the candidates with the exact softmax denominators */
#define FM_MODE_DENSE 2           /* float16 planes + the dense sum kernel (float32-equivalent product on the matrix
                                     cores) for the samples the screening kernel flags; both exit at once otherwise */
#define FM_MODE_NO_CELL_MAPS 4    /* skip the cell -> match maps of fm_coarse_cell_maps (two returning atomics per match):
                                     for callers that do not use the cell-ordered window crops */
#define FM_MODE_STATS 16          /* also leave the log-softmax offsets of EVERY row and column in the workspace
                                     (fm_coarse_softmax_stats): what fm_dual_softmax_conf_at / _backward read.  No
                                     row or column is skipped as "cannot hold a match"; needs the full-size workspace */
#define FM_MODE_EXACT_STEP 8      /* one more (small) kernel finds the largest |x| of every image first, and the int8
                                     screening step is derived from it instead of from a sample of rows: nothing is
                                     clipped, whatever the data (answers FM_E_STEP) */
#define FM_MODE_FLAT 32           /* a HINT (implies FM_MODE_DENSE): the caller expects flat similarity in every sample
                                     (an untrained network, textureless or occluded scenes - what FM_DEV_ALL_DENSE
                                     reported for the previous call of this kind).  The screening sweep, whose only
                                     finding would be "flat", is skipped: k_prep_split writes the float16 planes
                                     itself, a small kernel forms the stabilisers, and EVERY sample goes to the dense
                                     sum kernel - two launches and one pass over the descriptors fewer.  The hint never
                                     changes what is computed beyond which of the two float32-grade arithmetics serves
                                     a sample (they agree to ~1e-7): peaked data under the hint is correct, only slower */
#define FM_MODE_ALONE 64          /* a HINT about the DEVICE, not the data: this call has the GPU to itself (a single-pair
                                     caller on one stream - the reference's demo/demo.py:95-116).  Launches that cannot
                                     fill the chip then take the grid that is fastest for the kernel alone (two max-pass
                                     workgroups per compute unit, 8-unit screening chunks) instead of the smaller
                                     footprint that lets the kernels of OTHER pairs on other streams run beside them
                                     (the default: DESIGN.md section 5).  Results do not depend on it */

/* element type of the coarse descriptors handed to fm_coarse_match_dtype */
enum fm_dtype { FM_F32 = 0, FM_F16 = 1, FM_BF16 = 2 };

/* device status bits stored in d_count[1] */
#define FM_DEV_CAPACITY 1
#define FM_DEV_CANDIDATES 2
#define FM_DEV_RANGE 4
#define FM_DEV_DENSE 8
#define FM_DEV_INTERNAL 32
#define FM_DEV_STEP 128
#define FM_DEV_ALL_DENSE 256      /* informational, never an error: every sample of the call was served by the dense sum
                                     kernel (fm_read_count_info reports it; FM_MODE_FLAT is the faster way to run the
                                     next call on such data) */

int fm_version(void);
const char* fm_strerror(int status);

/* Candidate slots per coarse row the sparse assignment keeps: conf > thr implies
 * softmax(row) > thr, so at most ceil(1/thr)-1 entries of a row can qualify; the
 * default adds head-room for the float16 screening margin. */
int fm_default_cand_slots(float thr);

/* Bytes of device workspace fm_coarse_match needs (256-byte aligned base): fm_coarse_workspace_bytes for any mode and a
 * conf_matrix request, fm_coarse_workspace_bytes_mode for the given mode bits (want_conf_matrix != 0: as with
 * FM_MODE_DENSE | FM_MODE_EXACT_SCREENING); the common path (mode 0) needs about a quarter of the full size. */
int fm_coarse_workspace_bytes(int N, int L, int S, int C, int cand_slots, size_t* bytes);
int fm_coarse_workspace_bytes_mode(int N, int L, int S, int C, int cand_slots, int mode, int want_conf_matrix,
                                   size_t* bytes);

/*
 * Coarse stage (coarse_matching_new.py:43-143, eval mode).
 *   feat0 [N,L,C], feat1 [N,S,C]     [dev] float32, row-major (l = y*w0c + x)
 *   sim = feat0.feat1^T / (C*temperature); conf = softmax(sim,1)*softmax(sim,2)
 *   keep (b,i,j): conf > thr, both cells >= border_rm from their image border,
 *   conf == row max == column max; emitted sorted by (b,i,j) like torch.where.
 *   scale_px = hw0_i[0]/hw0_c[0] (:126); scale0/scale1 optional [dev] float32 [N,2]
 *   per-sample multipliers (:127-128) or NULL.
 * Outputs (capacity `cap` matches, all [dev]):
 *   b_ids,i_ids,j_ids int64[cap]; mkpts0_c,mkpts1_c float32[cap,2] (x,y px);
 *   mconf float32[cap]; d_count int32[2] = {M, status bits}.
 *   conf_matrix: optional [dev] float32 [N,L,S] (data['conf_matrix'], :70) or NULL.
 *   mode (the former exact_screening flag, same values for 0 / 1): 0 = the common path - prep, int8 max pass,
 *   screening kernel, assignment: candidates are screened in that sweep against lower bounds of the row / column
 *   maxima, which is enough for dual-softmax-trained descriptors; flat similarity reports FM_E_DENSE (a whole sample
 *   has no peaks) or FM_E_CANDIDATES (single rows overflow their cand_slots) through the status word.
 *   FM_MODE_DENSE adds the float16 planes and the dense sum kernel for flagged samples, FM_MODE_EXACT_SCREENING
 *   (implies FM_MODE_DENSE) two more kernels that repeat the screening with the exact softmax denominators, after
 *   which at most 1/thr entries of a row can be candidates; all of them are decided on the device and exit at once
 *   when not needed.  A conf_matrix request implies FM_MODE_DENSE (the sweep reads the float16 planes).  Every entry
 *   of the matrix is within 1e-5 of the float32 reference: entries on a screened sample's lists of significant entries,
 *   and the entries with conf > 0.1 of a sample with flat similarity together with the denominators that contain them,
 *   come from exact float32 dot products; for that the candidate lists of such a sample go down to min(thr, 0.1) - up
 *   to ~10 candidates per row: pass cand_slots >= 16 on flat data (fm_coarse_match_auto does).
 *   Shapes: any C % 4 == 0 in [4, 256] (the kernels work on planes zero-padded to 64, 128 or 256 channels; the workspace
 *   is that of the padded count, sim is divided by the caller's C) and any L, S >= 1; L and S may differ, and one-cell
 *   images are valid (the softmax over that image's side is then 1).  border_rm follows the reference's slicing
 *   (:11-28): 0 removes nothing, a border of at least half a grid side of either image removes every cell: M = 0, FM_OK.
 *   What the common path (mode 0) serves: its screening resolves at most 24 significant entries per 32 x 32 unit of the
 *   matrix and cand_slots per row / column, which peaked similarity on grids of 9 x 11 cells and more stays far below
 *   (a match per row: ~10 per unit at 99 cells, 0.2 at 4800).  It reports FM_E_DENSE, like any flat sample, for very
 *   few channels (C = 4, 12: no peaks) and for SMALL pairs whose significant entries crowd one unit: roughly 25 to 45
 *   cells per image with a partner for nearly every cell (the first unit then holds more than 24 matches), a one-cell
 *   image against more than cand_slots cells, and grids of that size with partner-less cells (each owns a significant
 *   entry, its maximum).  Larger grids with partner-less cells are not covered by this statement.  A call that wants every row's statistics (FM_MODE_STATS, a conf_matrix) of data with
 *   textureless rows reports FM_E_CANDIDATES unless it runs with FM_MODE_EXACT_SCREENING (fm_coarse_match_auto adds
 *   that bit to such requests itself).  tests/test_gpu_coarse_edges.py pins the cases of both answers.
 */
int fm_coarse_match(const float* feat0, const float* feat1, int N, int L, int S, int C,
                    int h0c, int w0c, int h1c, int w1c,
                    float temperature, float thr, int border_rm, float scale_px,
                    const float* scale0, const float* scale1,
                    void* workspace, size_t workspace_bytes, int cand_slots, int mode,
                    int64_t* b_ids, int64_t* i_ids, int64_t* j_ids,
                    float* mkpts0_c, float* mkpts1_c, float* mconf,
                    int cap, int32_t* d_count, float* conf_matrix, void* stream);

/*
 * The same stage for descriptors in float32, float16 or bfloat16 (in_dtype = enum fm_dtype; feat0/feat1 [dev]
 * [N,L,C] / [N,S,C] of that type, 8-byte aligned rows): what a PyTorch-ROCm backbone under autocast hands over,
 * without an up-cast pass in between.  Every half-precision value is exact in float32 and so is the product of
 * two of them, so the result equals fm_coarse_match on the up-cast tensors (the reference's float32 arithmetic on
 * the same numbers, coarse_matching_new.py:64-66).  fm_coarse_match(...) == fm_coarse_match_dtype(..., FM_F32, ...).
 * The workspace does not depend on the input type.
 */
int fm_coarse_match_dtype(const void* feat0, const void* feat1, int in_dtype, int N, int L, int S, int C,
                          int h0c, int w0c, int h1c, int w1c,
                          float temperature, float thr, int border_rm, float scale_px,
                          const float* scale0, const float* scale1,
                          void* workspace, size_t workspace_bytes, int cand_slots, int mode,
                          int64_t* b_ids, int64_t* i_ids, int64_t* j_ids,
                          float* mkpts0_c, float* mkpts1_c, float* mconf,
                          int cap, int32_t* d_count, float* conf_matrix, void* stream);

/*
 * fm_coarse_match_dtype + a SIDE JOB for callers that go on to fm_fine_match_maps with NCHW float32 fine maps (the
 * reference's layout, network/net.py:56-57): the channels-last copy of image 1's fine map that fm_fine_match_maps makes
 * as its first launch does not depend on the coarse stage at all, and the assignment kernel - 152 small, latency-bound
 * workgroups at 640x480 - leaves the memory system idle.  Here the transpose rides in the assignment kernel's launch as
 * a second workgroup role: one launch fewer per pair and the copy costs no time of its own.
 *   feat_f1 [dev] float32 [Nf, 64, Hf1, Wf1] (NCHW), scratch1 [dev] fm_fine_maps_scratch_bytes(..., layout 0) bytes,
 *   16-byte aligned; afterwards call fm_fine_match_maps with layout = FM_LAYOUT_NCHW_PREPARED and the same scratch.
 * Everything else as fm_coarse_match_dtype (same outputs, same status codes).
 */
int fm_coarse_match_maps(const void* feat0, const void* feat1, int in_dtype, int N, int L, int S, int C,
                         int h0c, int w0c, int h1c, int w1c,
                         float temperature, float thr, int border_rm, float scale_px,
                         const float* scale0, const float* scale1,
                         void* workspace, size_t workspace_bytes, int cand_slots, int mode,
                         int64_t* b_ids, int64_t* i_ids, int64_t* j_ids,
                         float* mkpts0_c, float* mkpts1_c, float* mconf,
                         int cap, int32_t* d_count, float* conf_matrix,
                         const float* feat_f1, int Nf, int Cf, int Hf1, int Wf1, void* scratch1, void* stream);

/*
 * ONE call for any data: CoarseMatching.forward is one call in the reference (coarse_matching_new.py:43-73), and so is
 * this.  fm_coarse_match / _dtype enqueue exactly the kernels `mode` names and report what the data would have needed
 * through the status word; this function runs the common path, reads that word (a host sync on `stream`, where the
 * reference's torch.where syncs, :109) and answers it by itself:
 *   flat similarity (FM_E_DENSE)          -> the dense sum kernel's part is ADDED to what the common path left in the
 *                                            workspace (float16 planes, dense sums, a second assignment launch: the
 *                                            max pass and the screening are not repeated)
 *   candidate-slot overflow (FM_E_CANDIDATES) -> 16 slots + FM_MODE_EXACT_STEP on dense data, then the exact
 *                                            re-screening (FM_MODE_EXACT_SCREENING), then more slots up to max_cand_slots
 *   clipped int8 step (FM_E_STEP)         -> FM_MODE_EXACT_STEP
 *   the assignment's bounded wait (FM_E_INTERNAL) -> once more
 * Returns FM_OK with *m_out = M (the outputs hold M matches), FM_E_CAPACITY with *m_out = the capacity the outputs need
 * (call again with larger buffers; exact ties can exceed N*min(L,S)), FM_E_RANGE for descriptors that are not finite
 * or out of range, an argument error, or a hipError_t.  Never FM_E_DENSE / FM_E_STEP; FM_E_CANDIDATES only when
 * max_cand_slots slots do not hold a row's candidates even after the exact re-screening (thr < 1 / max_cand_slots).
 *   workspace: fm_coarse_workspace_bytes_auto(N, L, S, C, max_cand_slots) bytes (any mode, max_cand_slots slots;
 *              max_cand_slots = 0 means 64); a smaller workspace is used as far as it goes (FM_E_WORKSPACE beyond).
 *   mode: the options that do not depend on the data (FM_MODE_NO_CELL_MAPS, FM_MODE_STATS); data-dependent bits are
 *         taken as the mode to START with (a caller that knows its data saves the first, failing attempt).
 *   conf_matrix: optional [dev] float32 [N,L,S] or NULL, as in fm_coarse_match.
 *   hint_io: optional HOST int32.  In: 0, or the value a previous call on data of this kind left there - the call
 *            then starts where that one ended (flat data: FM_MODE_FLAT, no screening sweep; ...).  Out: the mode bits
 *            (low byte) and the cand_slots the data asked for beyond the request's own default (second byte, 0 = none)
 *            that served this call, the slot count the serving attempt actually ran with (third byte, always set,
 *            ignored on input: the `cand_slots` to pass to fm_coarse_cell_maps / fm_coarse_softmax_stats for this
 *            workspace), and the number of coarse launch sequences it took (fourth byte, informational).  A hint is never wrong, only possibly slower
 *            than the common path: pass 0 every so often to find out whether the data has changed (the Python layer
 *            does, every 64th call of a shape).
 *   info_out: optional, the raw FM_DEV_* status bits of the attempt that served the call.
 * All other arguments as fm_coarse_match_dtype.
 */
int fm_coarse_workspace_bytes_auto(int N, int L, int S, int C, int max_cand_slots, size_t* bytes);
int fm_coarse_match_auto(const void* feat0, const void* feat1, int in_dtype, int N, int L, int S, int C,
                         int h0c, int w0c, int h1c, int w1c,
                         float temperature, float thr, int border_rm, float scale_px,
                         const float* scale0, const float* scale1,
                         void* workspace, size_t workspace_bytes, int max_cand_slots, int mode,
                         int64_t* b_ids, int64_t* i_ids, int64_t* j_ids,
                         float* mkpts0_c, float* mkpts1_c, float* mconf,
                         int cap, int32_t* d_count, float* conf_matrix,
                         int32_t* hint_io, int32_t* m_out, int32_t* info_out, void* stream);

/* Copy {M, status} to the host and wait for the stream (the one host sync of the
 * path, where the reference's torch.where syncs: coarse_matching_new.py:109).
 * Returns FM_OK or the error the status bits encode; *m_out is min(M, cap) on
 * success and the required capacity on FM_E_CAPACITY. */
int fm_read_count(const int32_t* d_count, int cap, int32_t* m_out, void* stream);
/* The same, and the raw device status bits (FM_DEV_*, the informational ones included) in *info_out. */
int fm_read_count_info(const int32_t* d_count, int cap, int32_t* m_out, int32_t* info_out, void* stream);

/*
 * Window crop (fine_preprocess.py:43-50): out[m, wy*W+wx, c] =
 * feat_f[b_ids[m], c, stride*y - pad + wy, stride*x - pad + wx] (0 outside the
 * map) with (y,x) = divmod(ids[m], w_c).  layout 0 = NCHW contiguous (the
 * reference's), 1 = NHWC (channels-last storage of the same tensor; with Cf = 64 and
 * W in {5,7} a copy in 16-byte chunks, one wave per window: a window row is W*256
 * contiguous bytes there).
 * The number of windows is min(*d_count, m_max) when d_count != NULL (device
 * side, no host sync), else m_max.  out [m_max, W*W, Cf] float32; rows at or beyond
 * that number are left untouched.  The counted rows must be valid (b in [0, N), id a
 * cell of the coarse grid): the crop does not check them.
 * Shapes: Cf <= 512, W <= 15, any stride >= 1, any pad >= 0, any w_c >= 1 (the grid may
 * overhang the map: windows wholly in the padding are all zero); layout 1 needs Cf % 4 == 0.
 * The NCHW crop outside the 64-channel fast path (float32, Cf = 64, W in {5,7}) stages one
 * window in LDS, W*W*(Cf+1)*4 bytes: beyond 64 KiB (e.g. W = 15 with Cf > 71, W = 7 with
 * Cf > 333) it answers FM_E_UNSUPPORTED - hand such a map over channels-last (layout 1),
 * which has no such limit.
 */
int fm_gather_windows(const float* feat_f, int N, int Cf, int Hf, int Wf, int layout,
                      int W, int stride, int pad, int w_c,
                      const int64_t* b_ids, const int64_t* ids,
                      const int32_t* d_count, int m_max, float* out, void* stream);
/* The same with the element type of the map as an argument (enum fm_dtype): float16 / bfloat16 maps - what a backbone
 * under autocast hands over (network/net.py:56-57) - are read as they are (every value is exact in float32), no up-cast
 * pass over the whole map in front of the crop.  out is float32 either way. */
int fm_gather_windows_dtype(const void* feat_f, int map_dtype, int N, int Cf, int Hf, int Wf, int layout,
                            int W, int stride, int pad, int w_c,
                            const int64_t* b_ids, const int64_t* ids,
                            const int32_t* d_count, int m_max, float* out, void* stream);

/*
 * Cell-ordered window crop for NCHW maps with Cf = 64 and W in {5,7}: one wave per coarse cell in raster
 * order, every XCD a contiguous band of the map (keeps the windows of image 1, whose list order is
 * scattered over the map, inside one L2).  cell_to_match [N, cell_pitch] int32 holds match index + 1 per
 * cell of THIS image (0 = unmatched); ties[0] = number of matches that lost their cell to an exactly
 * tied match, ties[1..] = their indices (at most 1023 listed; beyond that the kernel scans the match
 * list).  fm_coarse_cell_maps returns the maps and tie lists the coarse stage keeps in its workspace
 * (valid until the workspace is reused).  Same outputs as fm_gather_windows, rows at or beyond
 * min(*d_count, m_max) included: they are left untouched whatever the cell map and the tie list say
 * about them (this holds for fm_gather_merge_windows and fm_gather_windows_pair too).
 * FM_E_UNSUPPORTED when the shape is outside this path: call fm_gather_windows instead.
 */
int fm_coarse_cell_maps(void* workspace, int N, int L, int S, int C, int cand_slots,
                        int32_t** cell0, int* pitch0, int32_t** ties0,
                        int32_t** cell1, int* pitch1, int32_t** ties1);
int fm_gather_windows_cells(const float* feat_f, int N, int Cf, int Hf, int Wf, int W, int stride, int pad,
                            int h_c, int w_c, const int32_t* cell_to_match, int cell_pitch, const int32_t* ties,
                            const int64_t* b_ids, const int64_t* ids, const int32_t* d_count, int m_max,
                            float* out, void* stream);

/*
 * Window crop FUSED with the context merge of FinePreprocess (fine_preprocess.py:52-60,
 * fine_concat_coarse_feat = True - the reference's only working setting):
 *     out[m, r, :] = W_w . window[m, r, :] + ctx_bias[b_m, cell_m, :]
 * where merge_feat.weight = [W_w | W_c] ([64, 128]) and
 *     ctx_bias[b, cell, :] = W_c . (down_proj.weight . feat_c[b, cell, :] + down_proj.bias) + merge_feat.bias
 * is a per-cell table [N, h_c*w_c, 64] the caller computes with two plain GEMMs (it does not depend on the
 * window position).  The un-merged windows never reach memory.  packed_w = 16 KiB device buffer filled once
 * per weight update by fm_merge_pack_weights(merge_feat.weight [64,128] row-major).  The product runs as
 * hi/lo-split f16 MFMAs with f32 accumulation (f32-equivalent, ~2^-22 relative); the window operand carries a
 * power-of-two scale that follows every window's largest magnitude (any finite float32 map), the weights a fixed one:
 * |merge_feat.weight| < 16 (a larger weight is packed as NaN: the outputs it touches are NaN, never a wrong number).
 * cell_to_match / ties as in fm_gather_windows_cells, or both NULL for list order.  NCHW, Cf = 64, W in {5,7}.
 */
int fm_merge_pack_weights(const float* merge_w, int Cf, void* packed_w, void* stream);
int fm_gather_merge_windows(const float* feat_f, int N, int Cf, int Hf, int Wf, int W, int stride, int pad,
                            int h_c, int w_c, const int32_t* cell_to_match, int cell_pitch, const int32_t* ties,
                            const void* packed_w, const float* ctx_bias,
                            const int64_t* b_ids, const int64_t* ids, const int32_t* d_count, int m_max,
                            float* out, void* stream);

/*
 * Both images' crops in ONE launch (cell order; what FinePreprocess.forward does in a row,
 * fine_preprocess.py:43-50 / 52-60): out0 from feat_f0 / i_ids, out1 from feat_f1 / j_ids.
 * packed_w NULL = plain crop; non-NULL = crop fused with the context merge (ctx0/ctx1 required).
 * Each crop is bound by one round of memory latency at 640x480, so a second launch only adds ramp and tail.
 */
int fm_gather_windows_pair(const float* feat_f0, const float* feat_f1, int N, int Cf, int Hf0, int Wf0, int Hf1,
                           int Wf1, int W, int stride, int pad, int h0c, int w0c, int h1c, int w1c,
                           const int32_t* cell0, int pitch0, const int32_t* ties0,
                           const int32_t* cell1, int pitch1, const int32_t* ties1,
                           const void* packed_w, const float* ctx0, const float* ctx1,
                           const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids,
                           const int32_t* d_count, int m_max, float* out0, float* out1, void* stream);

/*
 * The crop fused with the context merge for CHANNELS-LAST maps: feat_f0 / feat_f1 are the storage
 * [N, Hf, Wf, 64] of the logical [N, 64, Hf, Wf] tensors, elements of map_dtype (enum fm_dtype: float16 /
 * bfloat16 maps are read as they are - every value is exact in float32 - no up-cast pass, no layout copy).
 * One launch serves both images: out0 from feat_f0 / i_ids / ctx0, out1 from feat_f1 / j_ids / ctx1.
 * feat_f1 == NULL means ONE image: feat_f1, ctx1, j_ids, out1, Hf1, Wf1, h1c and w1c are then ignored.
 * packed_w (fm_merge_pack_weights), ctx0 / ctx1 ([N, h0c*w0c, 64] / [N, h1c*w1c, 64]) and the arithmetic are
 * those of fm_gather_merge_windows: the outputs are bit-identical to that call on the same logical float32
 * tensor stored NCHW.  Windows are visited in list order (a channels-last window is W runs of W*256 contiguous
 * bytes wherever it lies: no cell map needed).  Rows at or beyond min(*d_count, m_max) are left untouched.
 * Cf = 64, W in {5,7}, any map_dtype of the enum; else FM_E_UNSUPPORTED.
 */
int fm_gather_merge_windows_nhwc(const void* feat_f0, const void* feat_f1, int map_dtype, int N, int Cf,
                                 int Hf0, int Wf0, int Hf1, int Wf1, int W, int stride, int pad,
                                 int h0c, int w0c, int h1c, int w1c,
                                 const void* packed_w, const float* ctx0, const float* ctx1,
                                 const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids,
                                 const int32_t* d_count, int m_max, float* out0, float* out1, void* stream);

/*
 * Fine stage (fine_matching_new.py:50-79): dual-direction window correlation,
 * softmax heat-map, spatial expectation, std.  win0/win1 [m_max, WW, Cf];
 * mix0/mix1 [dev] float32 [WW+1] = Linear(WW,1) weight then bias;
 * out0/out1 [m_max,3] = (x_px, y_px, std) with
 *   xy = mkpts_c + coords*(W/2)*scale_f + W/2        (:75-76)
 * d_count [dev] may be NULL: the list then has m_max rows.  Rows at or beyond min(*d_count, m_max) are left
 * untouched - out0 / out1 keep whatever they held - and nothing of those rows is read (windows, mkpts*_c);
 * *d_count = 0 writes nothing, m_max = 0 returns at once.  The counted rows do not depend on the count.
 */
int fm_fine_match(const float* win0, const float* win1, int m_max, const int32_t* d_count,
                  int WW, int Cf, const float* mix0, const float* mix1,
                  const float* mkpts0_c, const float* mkpts1_c, float scale_f,
                  float* out0, float* out1, void* stream);

/*
 * Training surface of the fine stage (the gradient of fine_matching_new.py:50-79 and of the crop,
 * fine_preprocess.py:43-50).  float32 arithmetic, no float atomics: both calls are bitwise reproducible.
 *
 *   fm_fine_match_backward : the gradient of fm_fine_match.  d_out0 / d_out1 [dev] float32 [m_max, 3] = dL/d out0 /
 *                            out1.  Per direction (0 shown; 1 swaps the windows), t = 1/sqrt(64), g = d_out0[m],
 *                            Wh = W/2, (gx, gy) = the normalised kornia grid, h = the forward's heat map (recomputed
 *                            with the forward's arithmetic), co / var its expectation and variance:
 *                              dvar_k = g[2] / (2 sqrt(var_k)) if var_k >= 1e-10 else 0,  dco_k = g[k] Wh scale_f - 2 co_k dvar_k
 *                              ds[r] = h[r] (dh[r] - sum h dh),  dh = dco_x gx + dco_y gy + dvar_x gx^2 + dvar_y gy^2
 *                              dq = t sum_r ds[r] win1[r,:];  d_win1[r,:] += t ds[r] q;  d_win0[r,:] += mix0[r] dq
 *                              d_mix0[r] = sum_m dq . win0[r,:],  d_mix0[WW] = sum_m sum_c dq
 *                            Outputs d_win0 / d_win1 [m_max, WW, Cf], d_mix0 / d_mix1 [WW+1] (weights, then bias), all
 *                            float32 [dev].  Rows at or beyond min(*d_count, m_max) (d_count may be NULL) get zero
 *                            gradients and are never read (win0, win1, d_out0, d_out1 may hold anything there); a
 *                            negative *d_count counts as 0.  With a count of 0 (or below) every d_win row is zero and
 *                            d_mix0 / d_mix1 are all zero.  A *d_count above m_max counts as m_max.  What the counted
 *                            rows get, and d_mix, are bit for bit what the call on those rows alone gives.
 *                            d_mix is reduced from per-match partials in a fixed order.  workspace:
 *                            fm_fine_match_backward_workspace_bytes(m_max, WW) bytes [dev], 256-byte aligned.
 *                            Cf = 64, WW in {25, 49} (else FM_E_UNSUPPORTED); m_max = 0: returns at once, nothing written.
 *   fm_gather_windows_backward : the adjoint of fm_gather_windows.  d_win [dev] float32 [m_max, W*W, Cf]; b_ids / ids as
 *                            in the crop; h_c, w_c = the coarse grid.  d_feat [dev] float32 [N, Cf, Hf, Wf] in `layout`
 *                            (0 = NCHW, 1 = channels-last): EVERY element is written, pixel (y, x) of sample b gets the
 *                            sum of d_win over every (match, window position) that read it, 0 where no window reads.
 *                            Window positions in the padding contribute nothing; rows whose (b, id) lies outside
 *                            [0, N) x [0, h_c*w_c) read nothing and are skipped.  Gather form (a CSR of matches per
 *                            (b, cell) in the workspace; each pixel sums its covering cells in row-major order and each
 *                            cell's matches in ascending index).  Rows at or beyond min(*d_count, m_max) (d_count
 *                            may be NULL) contribute nothing, as if the list ended there: *d_count = 0 gives an all-zero
 *                            d_feat.  workspace: fm_gather_windows_backward_workspace_bytes
 *                            bytes [dev], 256-byte aligned.  Any Cf <= 512, W <= 15 (else FM_E_UNSUPPORTED), any stride,
 *                            pad and layout (no LDS limit, no Cf % 4 rule here); m_max = 0: returns at once, d_feat
 *                            untouched.
 * Statuses: FM_E_NULL (a required pointer is NULL; d_count may be NULL), FM_E_SHAPE (m_max < 0, non-positive sizes),
 * FM_E_UNSUPPORTED, FM_E_WORKSPACE (too small or misaligned), or a hipError_t.  The *_workspace_bytes functions return 0
 * for invalid sizes.
 */
size_t fm_fine_match_backward_workspace_bytes(int m_max, int WW);
int fm_fine_match_backward(const float* win0, const float* win1, int m_max, const int32_t* d_count, int WW, int Cf,
                           const float* mix0, const float* mix1, float scale_f, const float* d_out0, const float* d_out1,
                           void* workspace, size_t workspace_bytes, float* d_win0, float* d_win1, float* d_mix0,
                           float* d_mix1, void* stream);
size_t fm_gather_windows_backward_workspace_bytes(int N, int h_c, int w_c, int m_max);
int fm_gather_windows_backward(const float* d_win, const int64_t* b_ids, const int64_t* ids, const int32_t* d_count,
                               int m_max, int N, int Cf, int Hf, int Wf, int layout, int W, int stride, int pad, int h_c,
                               int w_c, void* workspace, size_t workspace_bytes, float* d_feat, void* stream);

/*
 * Window crop + fine stage in one call, straight from the fine maps (fine_preprocess.py:43-50 with the plain
 * windows, then fine_matching_new.py:50-79): for callers without fine-level context layers between the two.  The
 * window tensors never exist: with channels-last maps (layout 1: [N,Hf,Wf,64] storage - a window row is W*256
 * contiguous bytes) every window position of both images is one coalesced 256-byte load of the kernel that does
 * the arithmetic of fm_fine_match.  layout 0 (NCHW, the reference's): the windows of image 0 are read from the
 * NCHW map as it is (the match list walks image 0 in raster order, which the NCHW window loader copes with); image 1,
 * whose windows land wherever the partners are, first gets a channels-last copy in `scratch`
 * (fm_fine_maps_scratch_bytes bytes [dev], 16-byte aligned; 0 bytes / NULL for layout 1) by a tiled transpose.  b_ids / i_ids / j_ids, d_count, mkpts*_c as the coarse stage left them; mix0 / mix1, scale_f,
 * out0 / out1 as in fm_fine_match.  Cf = 64, W in {5,7}.  Results equal fm_gather_windows + fm_fine_match bit for bit,
 * at any stride and pad, for any order of b_ids, and whether or not w0c / w1c times the stride equals the map (cells
 * beyond the map give zero windows).  The count as in fm_fine_match: d_count may be NULL; rows at or beyond
 * min(*d_count, m_max) are left untouched in out0 / out1 and their ids are not read; *d_count = 0 writes nothing (the
 * channels-last copies of layout 0 are still made).  The same holds for fm_fine_match_maps_dtype below and for
 * layout = FM_LAYOUT_NCHW_PREPARED.
 */
#define FM_LAYOUT_NCHW_PREPARED 2  /* layout of fm_fine_match_maps*: NCHW maps whose image-1 channels-last copy already sits in
                                     `scratch` - made by fm_coarse_match_maps, whose assignment launch carries the
                                     transpose as a side job (float32 maps) */
size_t fm_fine_maps_scratch_bytes(int N, int Cf, int Hf0, int Wf0, int Hf1, int Wf1, int layout);
int fm_fine_match_maps(const float* feat_f0, const float* feat_f1, int layout, int N, int Cf, int Hf0, int Wf0,
                       int Hf1, int Wf1, int W, int stride, int pad, int w0c, int w1c,
                       const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids,
                       const int32_t* d_count, int m_max, const float* mix0, const float* mix1,
                       const float* mkpts0_c, const float* mkpts1_c, float scale_f,
                       void* scratch, float* out0, float* out1, void* stream);

/*
 * The same with the element type of the maps as an argument (enum fm_dtype): FM_F16 / FM_BF16 maps - what a backbone
 * under autocast hands over (network/net.py:56-57) - are read as they are, no up-cast pass.  Every float16 /
 * bfloat16 value is exact in float32 and the arithmetic is the float32 call's, so the result equals
 * fm_fine_match_maps on the up-cast maps bit for bit.  layout 1: the 2-byte channels-last maps are read in place
 * (128 bytes per pixel).  layout 0 (NCHW): BOTH maps get channels-last copies in `scratch`, in their own element type
 * (half the bytes of the float32 route's copy); fm_fine_maps_scratch_bytes_dtype sizes it.
 */
size_t fm_fine_maps_scratch_bytes_dtype(int N, int Cf, int Hf0, int Wf0, int Hf1, int Wf1, int layout, int map_dtype);
int fm_fine_match_maps_dtype(const void* feat_f0, const void* feat_f1, int map_dtype, int layout, int N, int Cf, int Hf0,
                             int Wf0, int Hf1, int Wf1, int W, int stride, int pad, int w0c, int w1c,
                             const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const int32_t* d_count,
                             int m_max, const float* mix0, const float* mix1, const float* mkpts0_c,
                             const float* mkpts1_c, float scale_f, void* scratch, float* out0, float* out1, void* stream);

/*
 * Coarse-level context layers in front of the coarse matching (network/net.py:74): the reference's
 * LocalFeatureTransformer (network/module/transformer.py:34-57,78-96, attentions.py:19-46) in its default coarse
 * configuration - d_model 256, 8 heads, linear attention, no masks, any sequence of 'self' / 'cross' layers - on
 * feat0 [dev] float32 [N,L,256] and feat1 [N,S,256].  Float32 arithmetic on the float32 matrix cores; three launches
 * per encoder layer (K/V projection + per-tile KV partials, their fold, the fused query-side layer).
 * packed = fm_coarse_tf_packed_bytes(n_layers) bytes [dev], filled once per weight update by
 * fm_coarse_tf_pack_weights: layers[l] = HOST array of 10 DEVICE pointers in state-dict order - q_proj, k_proj,
 * v_proj, merge .weight [256,256]; mlp.0.weight [512,512]; mlp.2.weight [256,512]; norm1.weight, norm1.bias,
 * norm2.weight, norm2.bias [256].  layer_kinds [host] n_layers ints: 0 = 'self', 1 = 'cross'.  workspace [dev]
 * fm_coarse_tf_workspace_bytes(N, L, S) bytes, 16-byte aligned.  out0 / out1 must not alias the inputs.
 * FM_E_UNSUPPORTED for any other C / nhead / layer kind (the caller keeps its own layers then).
 */
size_t fm_coarse_tf_packed_bytes(int n_layers);
int fm_coarse_tf_workspace_bytes(int N, int L, int S, size_t* bytes);
int fm_coarse_tf_pack_weights(const float* const* const* layers, int n_layers, void* packed, void* stream);
int fm_coarse_transformer(const float* feat0, const float* feat1, int N, int L, int S, int C, int nhead,
                          const int* layer_kinds, int n_layers, const void* packed, void* workspace,
                          size_t workspace_bytes, float* out0, float* out1, void* stream);
/* The same with the reference's padding masks (transformer.py:78-96 mask0 / mask1; attentions.py:35-40: padded query
 * positions get Q = 0, padded source positions K = V = 0; values are still divided by the PADDED length): mask0 [N, L],
 * mask1 [N, S] [dev] bytes (1 = a real token, 0 = padding: torch.bool storage), either may be NULL. */
int fm_coarse_transformer_masked(const float* feat0, const float* feat1, const unsigned char* mask0,
                                 const unsigned char* mask1, int N, int L, int S, int C, int nhead,
                                 const int* layer_kinds, int n_layers, const void* packed, void* workspace,
                                 size_t workspace_bytes, float* out0, float* out1, void* stream);

/*
 * Fine-level context layers between the window crop and the fine matching (network/net.py:79-80): the reference's
 * LocalFeatureTransformer (network/module/transformer.py:34-57,78-96, attentions.py:19-46) in its default fine
 * configuration - d_model 64, 8 heads, layer_names ['self', 'cross'], linear attention, no masks - as ONE kernel,
 * one wave per match working on 32-token slices kept in registers from their load to their store, float32-equivalent
 * products (hi/lo-split float16 MFMAs).  win0/win1, out0/out1 [dev] float32 [m_max, WW, 64], WW in {25, 49}.  out0 /
 * out1 must not overlap win0, win1 or each other, in any byte (FM_E_UNSUPPORTED, nothing is written): a match that
 * lowers its scale is recomputed from its input windows, which the first pass would already have overwritten.  win0
 * and win1 are only read and may be one buffer.  Rows at or beyond min(*d_count, m_max) are left untouched (d_count may
 * be NULL; m_max = 0 writes nothing).  packed = fm_fine_tf_packed_bytes() bytes [dev] filled once per weight update by
 * fm_fine_tf_pack_weights(layer0, layer1, ...): each a HOST array of 10 DEVICE pointers in state-dict order -
 * q_proj, k_proj, v_proj, merge .weight [64,64]; mlp.0.weight [128,128]; mlp.2.weight [64,128]; norm1.weight,
 * norm1.bias, norm2.weight, norm2.bias [64] - of layers.0 ('self') and layers.1 ('cross').
 * Operand scales: weights x 2^12 (fixed: |w| < 16, checked by fm_fine_tf_pack_weights), activations x 2^8 and the
 * per-head sums of elu(k)+1 x 2^5 in float16 at the FIRST attempt - window values, their projections, the entries of
 * K^T V / S and the MLP's hidden layer below 255.9 in magnitude, sum_s (elu(k)+1) of a head feature below 2047
 * (LayerNorm-ed activations of a
 * trained network are O(1)).  The kernel FOLLOWS the largest magnitude that enters a float16 operand, per match; a
 * match that left the range is recomputed inside the kernel from its input windows with activation (and sum) scales
 * 16x, 256x, 4096x smaller (elements below 2^-3 / scale then lose the lo half of their split: three orders of
 * magnitude below the values that forced the scale down).  Only what does not fit at 2^-4 either (|activation| ~ 1e6,
 * NaN / Inf) or a weight >= 16 is reported: fm_fine_transformer_status ORs FM_DEV_RANGE into *d_status ([dev] int32,
 * zeroed by the caller) - the outputs are then not trustworthy and the caller must use float32 layers for this input
 * (the Python module does).  fm_fine_transformer is the same call without the report.  fm_coarse_transformer has no
 * such limit (its scales follow the data).
 */
size_t fm_fine_tf_packed_bytes(void);
int fm_fine_tf_pack_weights(const float* const* layer0, const float* const* layer1, void* packed, void* stream);
int fm_fine_transformer(const float* win0, const float* win1, int m_max, const int32_t* d_count, int WW, int Cf,
                        const void* packed, float* out0, float* out1, void* stream);
int fm_fine_transformer_status(const float* win0, const float* win1, int m_max, const int32_t* d_count, int WW, int Cf,
                               const void* packed, float* out0, float* out1, int32_t* d_status, void* stream);
/* The same with the FIRST attempt's activation scale chosen by the caller: start_log2_scale in {8, 4, 0, -4} (8 = the
 * default above).  d_lowered ([dev] int32, zeroed by the caller, or NULL) receives by how much the matches of this call
 * went below it (0, 4, 8 or 12 = the largest lowering of any match): a caller that feeds start - lowered back into its
 * next call on similar data (the Python module does) no longer pays for the repeated passes - 0.74 -> 0.45 ms at 3769
 * matches of a random-weight network whose activations leave 2^8 in nearly every workgroup.  A smaller starting scale
 * costs the precision a lowering costs (see above), nothing else. */
int fm_fine_transformer_start(const float* win0, const float* win1, int m_max, const int32_t* d_count, int WW, int Cf,
                              const void* packed, float* out0, float* out1, int32_t* d_status, int start_log2_scale,
                              int32_t* d_lowered, void* stream);

/*
 * Match post-processing (the step after the path; utils/metrics.py:33-81): squared symmetric epipolar distance
 * of every match against a relative pose, and a RANSAC-free inlier score per pair.
 *   mkpts0/mkpts1 [dev] float32 [m_max, kpt_stride] (x, y in pixels first; kpt_stride = 3 for the fine
 *   keypoints [M,3], 2 for plain [M,2]); m_bids [dev] int64 [m_max] (data['m_bids']); the number of matches is
 *   max(0, min(*d_count, m_max)) when d_count != NULL (d_count [dev]: a device address, as in fm_estimate_pose).
 *   T_0to1 [dev] float32 [N,4,4], K0/K1 [dev] float32 [N,3,3],
 *   row-major.  E = [t]x R (:65-66), points normalised by their intrinsics (:41-42),
 *   d = (p1.E p0)^2 (1/((E p0)_x^2 + (E p0)_y^2) + 1/((E^T p1)_x^2 + (E^T p1)_y^2))   (:47-56).
 * Outputs: epi_errs float32 [m_max] (data['epi_errs']); optional inlier uint8 [m_max] (d < inlier_thr) and
 * per_pair int32 [N,2] = {matches, inliers} per pair, which the caller zeroes beforehand (the kernel adds).
 * A row whose id lies outside [0, N) - compared as int64, as fm_estimate_pose compares it, so 2^32 + 1 is no pair -
 * gets epi_errs = NaN and inlier = 0 and is counted in no pair.  Rows behind the count are not written at all: a caller
 * who wants them to read as foreign rows fills epi_errs with NaN and inlier with 0 beforehand (post.epipolar_errors does).
 * Status: FM_OK at once for m_max == 0; then FM_E_NULL for a missing mkpts0, mkpts1, m_bids, T_0to1, K0, K1 or epi_errs;
 * then FM_E_SHAPE for m_max < 0, N <= 0 or kpt_stride < 2.
 */
int fm_epipolar_errors(const float* mkpts0, const float* mkpts1, int kpt_stride, const int64_t* m_bids,
                       const int32_t* d_count, int m_max, int N, const float* T_0to1, const float* K0,
                       const float* K1, float inlier_thr, float* epi_errs, unsigned char* inlier,
                       int32_t* per_pair, void* stream);

/*
 * Training surface of the coarse stage without any [N, L, S] array.  The reference's coarse loss
 * (losses/loss.py:27-67 with sparse_spvs, its default) reads data['conf_matrix'] at the supervised entries only.
 *   fm_coarse_softmax_stats   : [dev] pointers into the workspace of a fm_coarse_match call that ran with FM_MODE_STATS
 *                               (or a conf_matrix request): softmax(sim, dim 2)[b,i,j] = exp2(k2 x + nm_r[b*pitch_r + i]) /
 *                               sum_r[b*pitch_r + i], softmax(sim, dim 1)[b,i,j] = exp2(k2 x + nm_c[b*pitch_c + j]) /
 *                               sum_c[b*pitch_c + j], x = feat0[b,i] . feat1[b,j], k2 = log2(e) / (C temperature)
 *                               formed in float32 as (1.0f / ((float)C * temperature)) * 1.4426950408889634f - THESE
 *                               roundings: the stabilisers are -k2 x_max, and log2(e) / (C temperature) in one division is
 *                               one ulp away at C = 36 or 100, which leaves 4.6e-5 in a conf near 1 at |sim| ~ 160
 *                               (stabiliser and denominator kept apart: folded into one offset the float32 rounding
 *                               would cost 1e-5 of a conf near 1).  Valid while the workspace is.
 *   fm_dual_softmax_conf_at   : conf[e] = softmax(sim,1) * softmax(sim,2) at K entries (b_ids, i_ids, j_ids [dev] int64),
 *                               from exact float32 dot products (coarse_matching_new.py:64-68 restricted to the entries).
 *   fm_dual_softmax_backward  : d_feat0 [N,L,C], d_feat1 [N,S,C] = the gradient of sum_e g_e conf_e w.r.t. the
 *                               descriptors, given gc[e] = g_e * conf_e [dev] float32 [K]:
 *                                 dL/dsim_kl = 2 g c [kl supervised] - A_kl u_l - B_kl v_k,  u / v = column / row sums of g c
 *                               (A, B recomputed tile by tile from the statistics; float32 arithmetic).  workspace:
 *                               fm_dual_softmax_backward_workspace_bytes bytes [dev], 256-byte aligned.  feat0 / feat1
 *                               float32.  The listed entries' gc is added into the zeroed u and v, and their own terms
 *                               into the zeroed gradients (before the sweeps' sums are added on top), with float atomics:
 *                               K and K C of them, linear in K whatever K is (K <= N L S is not required; a triple listed
 *                               twice counts twice).  THREE or more entries in one row or one column are the only sums
 *                               whose order is not fixed: the first lands on 0 exactly and two commute.
 * What tests/test_gpu_dsm_grad.py establishes about these calls and the coarse loss below, with statistics made by the caller:
 *   - pitch_r >= L and pitch_c >= S may be any such value, the two independently; positions L .. pitch_r - 1 and S ..
 *     pitch_c - 1 of a row of the statistics are never read (they may hold NaN).  A smaller pitch is FM_E_SHAPE.
 *   - the statistics need not come from fm_coarse_match: any (nm, sum) with exp2(-nm) sum the softmax denominator serves,
 *     and a relative error delta of the denominators reaches the gradients as at most ~4 delta of the summed terms'
 *     magnitude (not of the gradient: on saturated problems the gradient is the small residue of those terms).
 *   - fm_dual_softmax_backward adds a triple once per time it is listed (three times the same (b, i, j, gc) = once with
 *     3 gc); lists with at most two entries per row and per column give the same bits on every call.  The coarse loss wants
 *     DISTINCT triples.
 *   - K = 0: fm_dual_softmax_conf_at returns FM_OK and writes nothing; fm_dual_softmax_backward writes exact zeros to all
 *     of d_feat0 / d_feat1 and does not look at the id and gc pointers.  A sample of the batch without an entry gets
 *     exact zeros; so does every call of fm_dual_softmax_backward_dense with G = 0.
 *   - nothing outside the buffers, the outputs and the stated workspace bytes is read or written; the workspace may hold
 *     anything on entry.
 */
int fm_coarse_softmax_stats(void* workspace, int N, int L, int S, int C, int cand_slots, const float** nm_r,
                            const float** sum_r, int* pitch_r, const float** nm_c, const float** sum_c, int* pitch_c);
int fm_dual_softmax_conf_at(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature,
                            const float* nm_r, const float* sum_r, int pitch_r, const float* nm_c, const float* sum_c,
                            int pitch_c, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int K,
                            float* conf, void* stream);
size_t fm_dual_softmax_backward_workspace_bytes(int N, int L, int S, int C);
int fm_dual_softmax_backward(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature,
                             const float* nm_r, const float* sum_r, int pitch_r, const float* nm_c, const float* sum_c,
                             int pitch_c, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const float* gc,
                             int K, void* workspace, size_t workspace_bytes, float* d_feat0, float* d_feat1, void* stream);
/* The same for a DENSE dL/dconf: G [dev] float32 [N, L, S] (the reference's loss terms over ALL negatives, losses/loss.py:
 * 44-50, 62-65, hand back a gradient for every entry).  conf is recomputed tile by tile from exact float32 dot products
 * and the statistics; three tiled sweeps (the row / column sums of G conf, then the two gradients) read G three times and
 * write nothing of its size: same workspace as fm_dual_softmax_backward, no [N, L, S] temporary.  No atomics: the row and
 * column sums are partials with one writer each (in the part of the workspace the gradient sweeps use afterwards), added up
 * in index order - the same bits on every run. */
int fm_dual_softmax_backward_dense(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature,
                                   const float* nm_r, const float* sum_r, int pitch_r, const float* nm_c, const float* sum_c,
                                   int pitch_c, const float* G, void* workspace, size_t workspace_bytes, float* d_feat0,
                                   float* d_feat1, void* stream);

/*
 * The reference's coarse loss over ALL entries of conf_matrix (losses/loss.py:44-50 cross entropy, :62-67 focal with
 * sparse_spvs = False) and its gradient w.r.t. the descriptors, without conf_matrix, conf_matrix_gt or any other
 * [N, L, S] array.  With c = clamp(conf, lo, hi) (lo, hi: the float32 roundings of 1e-6 and 1 - 1e-6, the bounds the
 * reference's float32 clamp uses), P the K supervised entries (b_ids, i_ids, j_ids [dev] int64, DISTINCT triples):
 *     loss = neg_weight / (N L S - K) * ( sum_all l_neg(c) - sum_P l_neg(c_e) ) + pos_weight / K * sum_P l_pos(c_e)
 *     FM_LOSS_CROSS_ENTROPY : l_pos = -log c,                         l_neg = -log(1 - c)
 *     FM_LOSS_FOCAL         : l_pos = -alpha (1 - c)^gamma log c,     l_neg = -alpha c^gamma log(1 - c)
 * conf is recomputed tile by tile from exact float32 dot products and the softmax statistics of the coarse call
 * (fm_coarse_softmax_stats), as in fm_dual_softmax_backward_dense; dloss/dconf is formed in registers.
 *   fm_coarse_loss_forward  : loss_out [dev] float32 [3] = {loss, mean of l_pos over P, mean of l_neg over the negatives}.
 *                             The loss is the same bits on every run (its sums are taken in a fixed order).  One sweep.
 *   fm_coarse_loss_backward : d_feat0 [N,L,C], d_feat1 [N,S,C] = d_loss[0] * dloss/dfeat; d_loss [dev] float32 [1] is read
 *                             on the device.  Same problem arguments as the forward call and ITS workspace, untouched
 *                             since.  Two sweeps; the same bits on every run, as fm_dual_softmax_backward_dense (with at
 *                             most two supervised entries per row and per column: see fm_dual_softmax_backward).
 * workspace: fm_coarse_loss_workspace_bytes bytes [dev], 256-byte aligned (0 for an invalid shape).  No host
 * synchronisation in either call.  K = 0 (the id pointers may be NULL) and K = N L S are the reference's degenerate cases
 * (loss.py:37-42): entry (0, 0, 0) stands in as the one positive with pos_weight 0 and, as in the reference, stays among
 * the N L S negatives; without a negative neg_weight counts as 0 and loss_out[2] is 0.  Statuses: FM_E_NULL, FM_E_SHAPE (K < 0, K > N L S, non-positive sizes, pitches below L / S),
 * FM_E_UNSUPPORTED (C, temperature <= 0, unknown kind, gamma <= 0), FM_E_WORKSPACE (too small / misaligned), a hipError_t.
 */
enum fm_loss_kind { FM_LOSS_CROSS_ENTROPY = 0, FM_LOSS_FOCAL = 1 };
size_t fm_coarse_loss_workspace_bytes(int N, int L, int S, int C, int K);
int fm_coarse_loss_forward(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature,
                           const float* nm_r, const float* sum_r, int pitch_r, const float* nm_c, const float* sum_c,
                           int pitch_c, int kind, float alpha, float gamma, float pos_weight, float neg_weight,
                           const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int K, void* workspace,
                           size_t workspace_bytes, float* loss_out, void* stream);
int fm_coarse_loss_backward(const float* feat0, const float* feat1, int N, int L, int S, int C, float temperature,
                            const float* nm_r, const float* sum_r, int pitch_r, const float* nm_c, const float* sum_c,
                            int pitch_c, int kind, float alpha, float gamma, float pos_weight, float neg_weight,
                            const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int K, void* workspace,
                            size_t workspace_bytes, const float* d_loss, float* d_feat0, float* d_feat1, void* stream);

/*
 * Ground-truth supervision from K correspondences (the reference's data_preprocess, datasets/data_preprocessing.py:9-64,
 * without its two host round trips).  kp0 / kp1 [dev] float32 [K, 2] = (x, y) in pixels, 8-byte aligned; the coarse grids
 * (h0c, w0c), (h1c, w1c); `cell` the cell size in pixels (8 in the reference).  Cell = floor(coord / cell) per axis.
 *   - Of all correspondences in one image-1 cell the one with the SMALLEST input index survives.
 *   - Survivors are emitted sorted by (cx1, cy1), cx1 the major key (np.unique(axis=0)'s order - not the order of j).
 *   - Survivor t: i_ids[t] = cx0 + cy0 w0c, j_ids[t] = cx1 + cy1 w1c (int64); coarse_kp0/1[t] = cell index * cell;
 *     fine_kp0/1[t] = the original points; lists_f0/1[t] = i, j as float32 (exact: a grid has at most 2^24 cells).  All
 *     [dev], `cap` rows, cap >= min(K, S).
 *   - fine_mtx_0 [L, 2], fine_mtx_1 [S, 2] (L = h0c w0c, S = h1c w1c): zero, then fine_mtx_1[j_t] = fine_kp1[t] (the j are
 *     distinct) and fine_mtx_0[i_t] = fine_kp0[t]; where several survivors share an i, the one with the LARGEST t wins.
 *   - d_count [dev] int32 [2] = {K', status} as fm_coarse_match leaves it: read it with fm_read_count.  A point whose cell
 *     lies outside its grid (negative, too large, NaN) sets FM_DEV_RANGE (fm_read_count: FM_E_RANGE) and is left out;
 *     nothing is wrapped or clamped.
 * Integer atomics only (min of the input index per image-1 cell, max of t per image-0 cell): every output is the same
 * bits on every run.  workspace: fm_supervise_workspace_bytes bytes [dev], 256-byte aligned (0 for an invalid grid).  No
 * host synchronisation.  K = 0 is valid (kp0 / kp1 and, with cap = 0, the per-survivor outputs may be NULL): K' = 0 and zero tables.
 * Statuses: FM_E_NULL, FM_E_SHAPE (K < 0, non-positive grid, cap < min(K, S)), FM_E_UNSUPPORTED (a grid of more than
 * 2^24 cells, cell <= 0 or not finite), FM_E_WORKSPACE, a hipError_t.
 */
size_t fm_supervise_workspace_bytes(int h0c, int w0c, int h1c, int w1c);
int fm_supervise_matches(const float* kp0, const float* kp1, int K, int h0c, int w0c, int h1c, int w1c, float cell,
                         void* workspace, size_t workspace_bytes, int64_t* i_ids, int64_t* j_ids, float* coarse_kp0,
                         float* coarse_kp1, float* fine_kp0, float* fine_kp1, float* lists_f0, float* lists_f1,
                         float* fine_mtx_0, float* fine_mtx_1, int cap, int32_t* d_count, void* stream);

/*
 * The reference's fine loss (Loss.compute_fine_loss, losses/loss.py:70-98) and its gradient.  expec0 / expec1 [dev]
 * float32, row m at expec + m * row_stride = (x, y, std) (row_stride >= 3 floats); gt0 / gt1 [dev] float32 [m_max, 2],
 * 8-byte aligned; d_count [dev] may be NULL as in fm_fine_match: rows at or beyond min(*d_count, m_max) are not read.
 * Per image, inv_m = 1 / max(std_m, 1e-10), nz = {m : gt[m, 0] != 0}, M = the rows counted:
 *     loss_d = sum_{m in nz} (|xy_m - gt_m|^2 / 49) inv_m / ((sum_all inv / M) |nz|),     loss_f = loss_0 + loss_1
 * If the sum of ALL entries of expec0 is exactly 0 (loss.py:72-75; decided on the device), loss_f = 0 with zero
 * gradients.  The sum is taken in double, the reference's in float32: entries that are not all zero and cancel only
 * through float32 rounding make the reference return 0 where this call computes the loss (entries that cancel exactly,
 * +a and -a, give 0 in both).  An empty nz gives NaN, as the reference's mean of an empty set; m_max = 0 gives 0
 * without a launch.
 *   fm_fine_loss_forward  : loss_out [dev] float32 [3] = {loss_f, loss_0, loss_1}.  Per-workgroup sums in double from
 *                           the first addition, folded in a fixed order: the same bits on every run.  Two launches.
 *   fm_fine_loss_backward : d_expec0 / d_expec1 [dev] float32 [m_max, 3], EVERY row written:
 *                             d expec[m, :2] = d_loss[0] 2 (xy_m - gt_m) / 49 inv_m / ((sum_all inv / M) |nz|) for m in nz,
 *                           0 for every other row and, the weights being detached, exactly 0 in the std column.  d_loss
 *                           [dev] float32 [1] is read on the device.  Same arguments as the forward call and ITS
 *                           workspace, untouched since (the reduced scalars and the row count are read from it).  One launch.
 * workspace: fm_fine_loss_workspace_bytes(m_max) bytes [dev], 256-byte aligned (0 for m_max < 0).  No atomics, no host
 * synchronisation.  Statuses: FM_E_NULL, FM_E_SHAPE (m_max < 0, row_stride < 3), FM_E_WORKSPACE, a hipError_t.
 */
size_t fm_fine_loss_workspace_bytes(int m_max);
int fm_fine_loss_forward(const float* expec0, const float* expec1, int row_stride, const float* gt0, const float* gt1,
                         int m_max, const int32_t* d_count, void* workspace, size_t workspace_bytes, float* loss_out,
                         void* stream);
int fm_fine_loss_backward(const float* expec0, const float* expec1, int row_stride, const float* gt0, const float* gt1,
                          int m_max, void* workspace, size_t workspace_bytes, const float* d_loss, float* d_expec0,
                          float* d_expec1, void* stream);

/*
 * Linear attention with the elu(x) + 1 feature map (the reference's LinearAttention, network/module/attentions.py:19-46)
 * and its gradient: the attention core of the context layers when they are trained.  q [dev] float32 [N, L, H*D], k / v
 * [dev] float32 [N, S, H*D], head h in channels [h*D, (h+1)*D), all (and d_out, state) 16-byte aligned; q_mask [dev] [N, L],
 * kv_mask [dev] [N, S]: one byte per token, 0 = padded (as fm_coarse_transformer_masked takes them), or NULL.  Per sample
 * and head, phi(x) = x + 1 for x > 0, else exp(x), Q = phi(q) q_mask, K = phi(k) kv_mask, V = v kv_mask:
 *     out[l] = (Q_l . sum_s K_s V_s^T) / (Q_l . sum_s K_s + eps)
 * (the reference's division of V by S and multiplication by S afterwards, a float16 precaution, is left out).  float32
 * arithmetic.  Two routes, chosen from the shape, both with H = 8:
 *     D = 8,  1 <= L, S <= 64 : one launch per call, one wave per sample; no state, no workspace (both byte queries
 *                               answer 0 and the two pointers may be NULL).  The fine level: [M, 25 | 49, 64].
 *     D = 32, L, S >= 1       : three launches per call (N <= 65535).  The coarse level: [N, 4800, 256].
 *   fm_linear_attention_forward  : out [dev] float32 [N, L, H*D]; `state` [dev] receives
 *                                  fm_linear_attention_state_bytes bytes (the K V^T and sum K of every sample and head).
 *   fm_linear_attention_backward : d_q [N, L, H*D], d_k, d_v [N, S, H*D] from d_out [N, L, H*D] and the `state` the
 *                                  forward call of the same arguments wrote.  Every element is written; the masks get
 *                                  no gradient.
 * workspace: fm_linear_attention_workspace_bytes bytes [dev], 256-byte aligned; the same size serves both calls and
 * nothing is kept in it between them.  Both byte queries answer 0 for a shape no route serves.  No atomics - every
 * output is the same bits on every run - and no host synchronisation or allocation.  Statuses: FM_E_NULL, FM_E_SHAPE (a
 * non-positive size), FM_E_UNSUPPORTED ((H, D, L, S) that neither route serves, eps <= 0), FM_E_WORKSPACE (too small /
 * misaligned), a hipError_t; every check returns before anything is launched.
 */
size_t fm_linear_attention_state_bytes(int N, int L, int S, int H, int D);
size_t fm_linear_attention_workspace_bytes(int N, int L, int S, int H, int D);
int fm_linear_attention_forward(const float* q, const float* k, const float* v, const unsigned char* q_mask,
                                const unsigned char* kv_mask, int N, int L, int S, int H, int D, float eps,
                                void* workspace, size_t workspace_bytes, float* state, float* out, void* stream);
int fm_linear_attention_backward(const float* q, const float* k, const float* v, const unsigned char* q_mask,
                                 const unsigned char* kv_mask, const float* d_out, const float* state, int N, int L,
                                 int S, int H, int D, float eps, void* workspace, size_t workspace_bytes, float* d_q,
                                 float* d_k, float* d_v, void* stream);

/*
 * Full softmax attention (the reference's FullAttention, network/module/attentions.py:48-79, without mask and dropout:
 * what its EncoderLayer constructs) and its gradient: the attention core of the context layers of attention = 'full'.
 * q, out, d_out, d_q [dev] float32 [N, L, H*D], k, v, d_k, d_v [dev] float32 [N, S, H*D], head h in channels
 * [h*D, (h+1)*D), all (and state) 16-byte aligned.  Per sample and head:
 *     out[l] = sum_s softmax_s(q_l . k_s / sqrt(D)) v_s
 * float32 arithmetic on the exact-float32 matrix instructions; the [L, S] scores of a head are never stored, forward
 * or backward.  Served: H = 8, D = 8 or 32, any L, S >= 1 (L != S: a cross layer between images of different size),
 * any N >= 1 while N * max(L, S) * H * D < 2^31 (N is not bounded by a grid dimension).
 *   fm_full_attention_forward  : out; online softmax over tiles of 32 keys (running maximum and sum).  `state` [dev], if
 *                                not NULL, receives fm_full_attention_state_bytes bytes: the log-sum-exp of the scaled
 *                                scores of every (n, h, l), float32 [N, H, L].  NULL is the inference call and writes
 *                                nothing.  One launch.
 *   fm_full_attention_backward : d_q, d_k, d_v from d_out, the forward call's `out` and the `state` it wrote (required).
 *                                The probabilities are recomputed from q, k and the state.  Three launches: delta =
 *                                rowsum(d_out * out) into the workspace, then d_k and d_v (a wave owns 32 keys and walks
 *                                the queries), then d_q (a wave owns 32 queries and walks the keys).
 * Every output element is written.  state: N*L*H floats rounded up to 256 bytes.  workspace:
 * fm_full_attention_workspace_bytes bytes [dev], 256-byte aligned (the same N*L*H floats: delta); both calls check it, the
 * backward call writes all of it before reading it and nothing is kept in it between calls.  Both byte queries answer 0
 * for an invalid or unserved shape.  No atomics and no sum across workgroups - every output is the same bits on every
 * call - and no host synchronisation or allocation.  Statuses, in this order and before anything is launched: FM_E_NULL
 * (q, k, v, out; backward: also d_out, state, d_q, d_k, d_v; the workspace when its byte query is non-zero), FM_E_SHAPE
 * (a non-positive size), FM_E_UNSUPPORTED (H != 8, D not 8 or 32, the element bound), FM_E_WORKSPACE (too small /
 * misaligned), a hipError_t.
 */
size_t fm_full_attention_state_bytes(int N, int L, int S, int H, int D);
size_t fm_full_attention_workspace_bytes(int N, int L, int S, int H, int D);
int fm_full_attention_forward(const float* q, const float* k, const float* v, int N, int L, int S, int H, int D,
                              void* workspace, size_t workspace_bytes, float* state, float* out, void* stream);
int fm_full_attention_backward(const float* q, const float* k, const float* v, const float* out, const float* d_out,
                               const float* state, int N, int L, int S, int H, int D, void* workspace,
                               size_t workspace_bytes, float* d_q, float* d_k, float* d_v, void* stream);

/*
 * The tail of an encoder layer of the context transformer (everything behind the attention) and its gradient, fused:
 * the fine level's training path, d = 64.  x, a [dev] float32 [T, d] (the layer's input and the attention's output, T
 * tokens, no token needs another); w_merge [d, d], w_mlp0 [2d, 2d], w_mlp2 [d, 2d] (nn.Linear weights, [out, in]);
 * ln1_w, ln1_b, ln2_w, ln2_b [d]; eps1, eps2 the LayerNorms' eps.  All pointers 16-byte aligned.  Per token:
 *     n1 = LN1(a w_merge^T)      o = max([x, n1] w_mlp0^T, 0) w_mlp2^T      y = x + LN2(o)
 * (biased variance).  float32 on the exact-float32 matrix instructions: one rounding per product, no reduced precision.
 *   fm_encoder_tail_forward  : y [dev] float32 [T, d].  Two launches.
 *   fm_encoder_tail_backward : d_x, d_a [T, d] and the seven parameter gradients, shaped as their parameters, from d_y
 *                              [T, d]; the forward chain is recomputed from x and a.  Every element is written.  The
 *                              seven parameter-gradient pointers are all non-NULL or all NULL; all NULL = d_x and d_a
 *                              only, and no parameter-gradient work is done.  Three launches (two without).
 * state: fm_encoder_tail_state_bytes answers 0 - nothing is kept between the calls - and `state` may be NULL.
 * workspace: fm_encoder_tail_workspace_bytes(T, d) bytes [dev], 256-byte aligned, at most 30 MiB whatever T is (the
 * weights in the kernels' operand order and one slab of partial parameter gradients per workgroup, at most 256); the same
 * size serves both calls and nothing is kept in it between them.  Supported: d = 64, 1 <= T <= 2^24 = 16 777 216.  Both
 * byte queries answer 0 for a shape that is not served.  No [T, d] or [T, 2d] intermediate reaches memory.  No atomics,
 * grids that depend on T alone: every output is the same bits on every run.  No host synchronisation or allocation.
 * Statuses, checked in this order before anything is launched: FM_E_NULL (a required pointer; some but not all of the
 * seven gradient pointers), FM_E_SHAPE (T <= 0 or d <= 0), FM_E_UNSUPPORTED (d != 64, an eps that is not > 0, T > 2^24),
 * FM_E_WORKSPACE (NULL, too small or misaligned); then a hipError_t.
 */
size_t fm_encoder_tail_state_bytes(int T, int d);
size_t fm_encoder_tail_workspace_bytes(int T, int d);
int fm_encoder_tail_forward(const float* x, const float* a, const float* w_merge, const float* ln1_w, const float* ln1_b,
                            const float* w_mlp0, const float* w_mlp2, const float* ln2_w, const float* ln2_b, int T, int d,
                            float eps1, float eps2, void* workspace, size_t workspace_bytes, float* state, float* y,
                            void* stream);
int fm_encoder_tail_backward(const float* x, const float* a, const float* w_merge, const float* ln1_w, const float* ln1_b,
                             const float* w_mlp0, const float* w_mlp2, const float* ln2_w, const float* ln2_b,
                             const float* d_y, const float* state, int T, int d, float eps1, float eps2, void* workspace,
                             size_t workspace_bytes, float* d_x, float* d_a, float* d_w_merge, float* d_ln1_w,
                             float* d_ln1_b, float* d_w_mlp0, float* d_w_mlp2, float* d_ln2_w, float* d_ln2_b,
                             void* stream);

/*
 * The same tail and its gradient at d = 256: the coarse level's training path.  Arguments, shapes (w_merge [256, 256],
 * w_mlp0 [512, 512], w_mlp2 [256, 512], the LayerNorm vectors [256]), alignment and arithmetic are those of
 * fm_encoder_tail_* above: float32 on the exact-float32 matrix instructions, one rounding per product, no reduced
 * precision, no BLAS call.
 *   fm_coarse_tail_forward  : y [dev] float32 [T, d].
 *   fm_coarse_tail_backward : d_x, d_a [T, d] and the seven parameter gradients from d_y [T, d]; the forward chain is
 *                             recomputed from x and a.  Every element is written.  The seven parameter-gradient pointers
 *                             are all non-NULL or all NULL; all NULL = d_x and d_a only, and no parameter-gradient work.
 * T is walked in chunks of at most 8192 tokens inside the call (5 launches per chunk forward, 14 backward, 9 without
 * parameter gradients); a chunk's [tokens, 256] and [tokens, 512] intermediates live in the workspace.
 * state: fm_coarse_tail_state_bytes answers 0 - nothing is kept between the calls - and `state` may be NULL.
 * workspace: fm_coarse_tail_workspace_bytes(T, d) bytes [dev], 256-byte aligned: one chunk's intermediates, one slab of
 * partial weight gradients per 512 tokens of a chunk and one row of partial LayerNorm gradients per 64.  It grows with T up
 * to 8192 tokens and is the same from there on (under 96 MiB); the same size serves both calls and nothing is kept in it
 * between them, nor is anything asked of its contents.  Supported: d = 256, 1 <= T <= 2^24.  Both byte queries answer 0
 * for a shape that is not served.  No atomics, grids that depend on T alone: every output is the same bits on every run.
 * No host synchronisation or allocation; everything goes to `stream` and can be captured in a graph.
 * Statuses, checked in this order before anything is launched: FM_E_NULL (a required pointer; some but not all of the
 * seven gradient pointers), FM_E_SHAPE (T <= 0 or d <= 0), FM_E_UNSUPPORTED (d != 256, an eps that is not > 0, T > 2^24),
 * FM_E_WORKSPACE (NULL, too small or misaligned); then a hipError_t.
 */
size_t fm_coarse_tail_state_bytes(int T, int d);
size_t fm_coarse_tail_workspace_bytes(int T, int d);
int fm_coarse_tail_forward(const float* x, const float* a, const float* w_merge, const float* ln1_w, const float* ln1_b,
                           const float* w_mlp0, const float* w_mlp2, const float* ln2_w, const float* ln2_b, int T, int d,
                           float eps1, float eps2, void* workspace, size_t workspace_bytes, float* state, float* y,
                           void* stream);
int fm_coarse_tail_backward(const float* x, const float* a, const float* w_merge, const float* ln1_w, const float* ln1_b,
                            const float* w_mlp0, const float* w_mlp2, const float* ln2_w, const float* ln2_b,
                            const float* d_y, const float* state, int T, int d, float eps1, float eps2, void* workspace,
                            size_t workspace_bytes, float* d_x, float* d_a, float* d_w_merge, float* d_ln1_w,
                            float* d_ln1_b, float* d_w_mlp0, float* d_w_mlp2, float* d_ln2_w, float* d_ln2_b,
                            void* stream);

/*
 * The q / k / v projections of an encoder layer of the context transformer (the three bias-free linear maps in front of
 * the attention) and their gradient, fused: the fine level's training path, d = 64.  x [dev] float32 [Tx, d] (the layer's
 * input), src [dev] float32 [Ts, d] (the tokens it attends to), wq, wk, wv [d, d] (nn.Linear weights, [out, in]).  All
 * pointers 16-byte aligned.
 *     q = x wq^T        k = src wk^T        v = src wv^T
 * float32 on the exact-float32 matrix instructions: one rounding per product, no reduced precision.
 * Self mode is src == x (the same address; then Ts must equal Tx): x is read once per pass.  Any other src is cross mode,
 * Tx and Ts independent.  Outputs must not overlap inputs or each other: that is the caller's duty and is not checked.
 *   fm_qkv_projection_forward  : q [Tx, d], k, v [Ts, d].  Two launches.
 *   fm_qkv_projection_backward : from gq [Tx, d], gk, gv [Ts, d] (the gradients of q, k, v):
 *                                  cross mode  d_x [Tx, d] = gq wq,  d_src [Ts, d] = gk wk + gv wv;
 *                                  self mode   d_x [Tx, d] = gq wq + gk wk + gv wv, one sum in registers; d_src is not
 *                                              written and may be NULL;
 *                                  d_wq = sum_t gq^T x,  d_wk = sum_t gk^T src,  d_wv = sum_t gv^T src, each [d, d].
 *                                Every element is written.  d_wq, d_wk, d_wv are all given or all NULL; all NULL = the
 *                                data gradients only, and no weight-gradient work is done.  Three launches (two without).
 * workspace: fm_qkv_projection_workspace_bytes(Tx, Ts, d) bytes [dev], 256-byte aligned, at most 13 MiB whatever the
 * token counts are (the weights in the kernels' operand order and one slab of partial weight gradients per workgroup, at
 * most 256); the same size serves both calls and both modes, and nothing is kept in it between calls.  Supported: d = 64,
 * 1 <= Tx, Ts <= 2^24 = 16 777 216.  The query answers 0 for arguments that the calls refuse.  No atomics, grids that
 * depend on Tx, Ts and the mode alone: every output is the same bits on every run.  No host synchronisation and no
 * allocation.
 * Statuses, checked in this order before anything is launched: FM_E_NULL (a required pointer; some but not all of d_wq,
 * d_wk, d_wv; d_src in cross mode), FM_E_SHAPE (Tx, Ts or d <= 0; src == x with Ts != Tx), FM_E_UNSUPPORTED (d != 64, a
 * token count above 2^24), FM_E_WORKSPACE (NULL, too small or misaligned); then a hipError_t.
 */
size_t fm_qkv_projection_workspace_bytes(int Tx, int Ts, int d);
int fm_qkv_projection_forward(const float* x, const float* src, const float* wq, const float* wk, const float* wv, int Tx,
                              int Ts, int d, void* workspace, size_t workspace_bytes, float* q, float* k, float* v,
                              void* stream);
int fm_qkv_projection_backward(const float* x, const float* src, const float* wq, const float* wk, const float* wv,
                               const float* gq, const float* gk, const float* gv, int Tx, int Ts, int d, void* workspace,
                               size_t workspace_bytes, float* d_x, float* d_src, float* d_wq, float* d_wk, float* d_wv,
                               void* stream);

/*
 * Window crop + context merge of the fine preprocessing (the crop, then the merge layer over [window | context]) and its
 * gradient, fused, per image: the fine level's training path.  feat_f [dev] float32 [N, Cf, Hf, Wf] in `layout` 0 (NCHW)
 * or 1 (channels-last); b_ids, ids [dev] int64 [m_max], (y, x) = divmod(ids[m], w_c) on the h_c x w_c coarse grid; w_win
 * [64, 64] float32 row-major ([out, in]: the merge weight's columns of the window half, contiguous); ctx [m_max, 64]
 * float32, the position-independent half of the merge, one row per match.  All pointers 16-byte aligned.
 *     win[m, r, c] = feat_f[b_m, c, stride y - pad + r / W, stride x - pad + r % W]     (0 outside the map)
 *     out[m, r, :] = w_win win[m, r, :] + ctx[m, :]                                     out [m_max, W W, 64]
 * float32 on the exact-float32 matrix instructions: one rounding per product, no reduced precision.  The windows and the
 * concatenation are never written to memory, in either direction.  The rows must be valid, as for fm_gather_windows: a
 * row whose sample or cell lies outside the batch or the grid reads a window of zeros (out = ctx[m]) and gives the map
 * no gradient, but nothing checks that a valid cell is the intended one.
 *   fm_window_merge_forward  : out.  Two launches.
 *   fm_window_merge_backward : from g [m_max, W W, 64] (the gradient of out):
 *                                d_ctx [m_max, 64]    = sum_r g[m, r, :];
 *                                d_w_win [64, 64]     = sum_{m, r} g[m, r, :]^T win[m, r, :] (the windows cropped again);
 *                                                       may be NULL: no weight-gradient work is done then;
 *                                d_feat [N, Cf, Hf, Wf] in `layout` = the crop's adjoint of g w_win, as
 *                                                       fm_gather_windows_backward defines it (every element written,
 *                                                       exact +0 where no window reads); may be NULL (a frozen
 *                                                       backbone): g w_win is not computed then.
 * workspace: fm_window_merge_workspace_bytes(N, h_c, w_c, m_max, W) bytes [dev], 256-byte aligned: the weight in the
 * kernels' operand order, one slab of partial weight gradients per workgroup (at most 256), g w_win [m_max, W W, 64] and
 * the crop backward's lists; the same size serves both calls, and nothing is kept in it between calls.  Supported: Cf =
 * 64, W in {5, 7}, stride >= 1, pad >= 0, m_max W W <= 2^24, fewer than 2^31 - 1 cells in the batch.  The query answers 0
 * for arguments that the calls refuse.  No float atomics, grids that depend on the arguments alone: every output is the
 * same bits on every run.  No host synchronisation and no allocation.
 * m_max = 0 returns FM_OK at once, nothing looked at or written.  Statuses, checked in this order before anything is
 * launched: FM_E_NULL (a required pointer; d_feat and d_w_win may be NULL), FM_E_SHAPE (a non-positive size or stride, m_max < 0),
 * FM_E_UNSUPPORTED (anything outside the list above, a layout that is neither 0 nor 1), FM_E_WORKSPACE (NULL, too small
 * or misaligned); then a hipError_t.
 */
size_t fm_window_merge_workspace_bytes(int N, int h_c, int w_c, int m_max, int W);
int fm_window_merge_forward(const float* feat_f, int N, int Cf, int Hf, int Wf, int layout, int W, int stride, int pad,
                            int h_c, int w_c, const float* w_win, const float* ctx, const int64_t* b_ids,
                            const int64_t* ids, int m_max, void* workspace, size_t workspace_bytes, float* out, void* stream);
int fm_window_merge_backward(const float* feat_f, int N, int Cf, int Hf, int Wf, int layout, int W, int stride, int pad,
                             int h_c, int w_c, const float* w_win, const float* ctx, const int64_t* b_ids,
                             const int64_t* ids, int m_max, const float* g, void* workspace, size_t workspace_bytes,
                             float* d_feat, float* d_w_win, float* d_ctx, void* stream);

/*
 * Relative pose of every pair from its matches (utils/metrics.py:79-109 estimate_pose, there OpenCV on the host, one pair
 * at a time): five-point RANSAC over `samples` hypotheses per pair, float64 arithmetic, four launches, no host
 * synchronisation.  Inputs as fm_epipolar_errors takes them: mkpts0 / mkpts1 [dev] float32 [m_max, kpt_stride], m_bids
 * [dev] int64 [m_max], the number of matches min(*d_count, m_max) when d_count != NULL, K0 / K1 [dev] float32 [N, 3, 3].
 *   m_bids must be NON-DECREASING (CoarseMatching writes it so): pair b owns a contiguous range of rows; a row whose id lies
 *   outside [0, N) belongs to no pair and its inlier flag is 0.
 *   Normalisation: q = ((x - cx) / fx, (y - cy) / fy), each image by its own K; a match is an inlier of E where its
 *   squared Sampson distance (q1^T E q0)^2 / ((E q0)_x^2 + (E q0)_y^2 + (E^T q1)_x^2 + (E^T q1)_y^2) is below
 *   (pixel_thr / f)^2, f = (fx0 + fy0 + fx1 + fy1) / 4.
 *   Sampling: draw k = 0..7 of hypothesis h of pair b is splitmix64((8 h + k) * 0x9E3779B97F4A7C15 + key) mod M_b with key
 *   = synth._stream_key(seed, b); the sample is the first five distinct draws (fewer, or M_b < 5: no hypothesis).
 *   Each sample yields up to ten essential matrices (Nister's five-point method); the pair's winner has the most inliers,
 *   then the lowest hypothesis, then the lowest candidate slot (ascending z).  Of its four decompositions (R, +-t) the one
 *   with the most inliers in front of both cameras wins, the first of equals.  The same inputs give the same bits.
 * Outputs [dev]: R_out float64 [N, 9] (row-major rotation), t_out float64 [N, 3] (unit length), E_out float64 [N, 9] (the
 * winning essential matrix, unit Frobenius norm), inlier uint8 [m_max] (the winner's inliers; every row is written),
 * per_pair int32 [N, 4] = {matches, inliers, inliers in front of both cameras, ok}.  ok = 1 only where the pair has at
 * least 5 matches, a candidate existed and some inlier lies in front of both cameras; else R = I, t = 0.
 * workspace: fm_pose_workspace_bytes(N, m_max, samples) bytes [dev], 256-byte aligned (the query returns 0 for what the
 * call refuses and does not decrease in any argument).
 * Statuses, checked in this order before anything is launched: FM_E_NULL (a required pointer; d_count may be NULL),
 * FM_E_SHAPE (N <= 0, m_max < 0, kpt_stride < 2, samples <= 0), FM_E_UNSUPPORTED (pixel_thr <= 0 or not finite, samples >
 * 65536, m_max >= 2^31 / 8), FM_E_WORKSPACE (NULL, too small or misaligned); then m_max = 0 returns FM_OK at once, nothing
 * written; then a hipError_t.
 */
size_t fm_pose_workspace_bytes(int N, int m_max, int samples);
int fm_estimate_pose(const float* mkpts0, const float* mkpts1, int kpt_stride, const int64_t* m_bids, const int32_t* d_count,
                     int m_max, int N, const float* K0, const float* K1, float pixel_thr, int samples, uint64_t seed,
                     void* workspace, size_t workspace_bytes, double* R_out, double* t_out, double* E_out,
                     unsigned char* inlier, int32_t* per_pair, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FMATCH_H_ */
