/* jds.h — C-ABI of the MI355X-native JPEG-DSP-Studio block-DCT codec path.
 *
 * The reference (Xneonz0/JPEG-DSP-Studio) is pure Python and has no FFI; its
 * boundary is the Python function engines.pipeline.compress_reconstruct
 * (engines/pipeline.py:17-21) plus the per-stage functions re-exported by
 * engines/__init__.py:10-27.  This library is what sits UNDER that boundary:
 * the drop-in Python package (jpeg-dsp-studio_amd/engines) binds these entry
 * points with ctypes (jpeg-dsp-studio_amd/jds/_abi.py).
 *
 * Conventions: plain pointers and sizes, no torch/HIP types in signatures
 * (streams are passed as void*).  Every int-returning function returns
 * JDS_OK (0) or a negative code; jds_last_error() holds a thread-local message.
 * All GPU work is hand-written HIP for gfx950; there is no CPU fallback.
 */
#ifndef JDS_H
#define JDS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JDS_ABI_VERSION 3

#define JDS_OK       0
#define JDS_EINVAL  (-1)  /* bad argument                    -> ValueError   */
#define JDS_ENOTSUP (-2)  /* e.g. block_size not 8/16          -> ValueError   */
#define JDS_EHIP    (-3)  /* HIP runtime / device failure     -> RuntimeError */
#define JDS_ENOMEM  (-4)  /* device allocation failed         -> RuntimeError */

/* subsampling modes: models/compression_params.py:13 ('4:4:4','4:2:2','4:2:0') */
#define JDS_SS_444 0
#define JDS_SS_422 1
#define JDS_SS_420 2
#define JDS_SS_GRAY 3 /* one-component (grayscale) files: jds_jpeg_parse and the calls on foreign files only */

/* jds_plan_run flags */
#define JDS_RUN_SSE 1u  /* fill sse_rgb / sse_y (PSNR); the inverse kernel re-reads the input */
#define JDS_RUN_FWD 2u  /* forward phase only (stats reset + k_fwd); with neither FWD nor INV: both */
#define JDS_RUN_INV 4u  /* inverse phase only (k_inv + finalize); needs the forward's coeffs/stats.  The
                           coefficients are the caller's: the certified fast inverse bounds |q Q| from
                           the values it reads.  Only a run of both phases in one call (8x8 blocks,
                           tiled geometry) certifies with the fixed bound |q Q| <= 1152 that holds
                           for its own forward's output */
#define JDS_RUN_EXACT 8u /* all-fp64 kernels (default: certified fp32 + exact fp64 fix-up, same results) */
#define JDS_RUN_EXACT_INV 16u /* inverse only: the replayed-order fp64 kernel instead of the certified fast
                                 inverse + tile fix-up (same bytes; A/B and tests) */
#define JDS_RUN_INV_FIXALL 32u /* test: the certified fast inverse flags every tile, so the exact
                                  tile code recomputes the whole frame (exercises the fix-up path) */
#define JDS_RUN_INV_FAST 128u /* A/B and tests, plans whose tables are all coarse (DC quantiser > 60): the
                                certified fast inverse instead of the exact k_inv2 such plans run (most
                                tiles of those frames fall back).  The 4:2:x kernel
                                then works as on any plan: an item whose previous fast run recomputed more
                                than 1/8 of its tiles runs the exact tile code directly (per-item exact
                                mode) until the next probe run, every 16th fast inverse of the plan.
                                Plans with some coarse and some finer tables take the fast inverse
                                without this flag, their coarse items in exact mode from the first run */
#define JDS_RUN_FWD_FIXALL 64u /* test, 16x16 plans: the certified fp32 forward lists every block, so
                                  k_fix_fwd16 recomputes the whole frame (exercises the fix-up path) */

/* `after` argument of the *_dev functions below: no wait, the caller has
 * synchronised the inputs.  (NULL is the HIP null stream, which is waited for.) */
#define JDS_AFTER_NONE ((void*)(intptr_t)-1)

typedef struct jds_ctx jds_ctx;    /* one per (thread, device): owns a HIP stream + scratch */
typedef struct jds_plan jds_plan;  /* fixed geometry + per-frame quant tables, device-resident */

/* Per-frame parameters.  Mirrors CompressionParams (models/compression_params.py:7-20);
 * the tables are computed on the host exactly as the reference does. */
typedef struct {
  /* 8: the reference's path.  16: the BASELINE configs[4] stretch the reference
   * stubs (models/compression_params.py:19-20 accepts it, engines/quantizer.py:24
   * then fails); its table is np.kron(qtable, ones((2, 2))), i.e.
   * Q16[u][v] = qtable[(u/2)*8 + v/2] (build decision).  Other values
   * fail with the reference's broadcast error (JDS_ENOTSUP). */
  int32_t block_size;
  int32_t quality;     /* 1..100 (informational; the table below is authoritative) */
  int32_t subsampling; /* JDS_SS_* */
  int32_t prefilter;   /* 0/1; ignored for 4:4:4 (engines/color_space.py:34-35) */
  double qtable[64];   /* scale_quant_matrix(JPEG_LUMA_Q50, quality) (engines/quantizer.py:7-19) */
  /* The prefilter's taps: cv2.getGaussianKernel(3, 0.75) in the reference
   * (engines/color_space.py:39-40).  Read only where the prefilter runs
   * (prefilter != 0 and not 4:4:4); there they must be finite with gauss[0] ==
   * gauss[2] (JDS_EINVAL otherwise, from every entry point that takes them):
   * the column pass is cv2's symmetric form k1 T[y] + k0 (T[y+1] + T[y-1]),
   * which has no definition for asymmetric taps.  Signs and sum are free; a
   * full run keeps its fixed |q Q| <= 1152 certificate (jds_plan_fix_counts)
   * only for non-negative taps whose sum is at most 1 and tracks the bound
   * otherwise, and taps whose sum is not 1 send every chroma block through
   * the forward's exact fix-up.  Same bytes either way. */
  double gauss[3];
} jds_params;

/* Per-frame statistics, all exact integers; sse_y is an exact integer sum
 * converted to double and divided by 1e6.
 * estimate_bitrate_no_entropy (utils/metrics.py:51-92), histogram
 * (engines/pipeline.py:123-124) and the PSNR sums (utils/metrics.py:11,20). */
typedef struct {
  uint64_t nonzero;             /* count of q != 0 */
  uint64_t total_coeffs;        /* all_quantized_coeffs.size */
  uint64_t magnitude_bits;      /* sum over q != 0 of ceil(log2(|q|+1)) + 1 */
  uint64_t block_overhead_bits; /* 2 * ceil(H/B) * ceil(W/B) (luma grid only) */
  uint64_t hist[50];            /* np.histogram(q, bins=50, range=(-100, 100))[0] */
  uint64_t sse_rgb;             /* sum (orig - rec)^2 over H*W*3 uint8 samples (JDS_RUN_SSE) */
  double sse_y;                 /* sum (Y(orig) - Y(rec))^2, Y = .299R+.587G+.114B (JDS_RUN_SSE):
                                   sum of (299dR+587dG+114dB)^2 in 64-bit integers / 1e6 */
  uint64_t pixels;              /* H * W */
  double fwd_ms, inv_ms;        /* host path only: forward / inverse kernel time (hipEvents) */
  double ssim[4];               /* host path only: SSIM of R, G, B and of Y (utils/metrics.py:12-21) */
  double mse_y;                 /* host path only: NumPy-order mean of (Y(orig) - Y(rec))^2 */
  double magnitude_bits_f32;    /* host path only: magnitude_bits as NumPy's float32 np.sum yields it */
  uint64_t reserved[1];
} jds_frame_stats;

typedef struct {
  int64_t H, W;
  int64_t chroma_h, chroma_w;        /* after subsampling, before padding */
  int64_t y_blocks_y, y_blocks_x;    /* padded luma block grid */
  int64_t c_blocks_y, c_blocks_x;    /* padded chroma block grid (per plane) */
  int64_t coeffs_per_frame;          /* B*B * (Y blocks + 2 * chroma blocks) */
  int64_t cb_offset, cr_offset;      /* coefficient offsets of the Cb / Cr planes */
  int32_t tiles, threads_fwd, threads_inv, reserved;
} jds_geometry;

/* IntermediateData.selected_block_* (engines/pipeline.py:128-151); 8x8 path only
 * (with block_size 16, *sel_valid is always 0) */
typedef struct {
  double original[64], shifted[64], dct[64];
  int16_t quantized[64];
  double dequantized[64], reconstructed[64];
} jds_selected_block;

int jds_abi_version(void);
const char* jds_last_error(void);
int jds_device_count(int* n);

/* Geometry of one frame (host only, no device access). */
int jds_geometry_of(const jds_params* p, int64_t H, int64_t W, jds_geometry* out);

int jds_ctx_create(int device, jds_ctx** out);
void jds_ctx_destroy(jds_ctx* ctx);
void* jds_ctx_stream(jds_ctx* ctx);  /* the context's own hipStream_t */
/* SSIM scratch budget per luma launch group of jds_psnr_ssim_batch_dev (bytes;
 * <= 0: the default 16 GB).  The group size follows from it; the scratch is
 * sized for the groups that run (a single pair beyond the budget still runs). */
int jds_ctx_set_ssim_scratch(jds_ctx* ctx, int64_t bytes);

/* Device-resident batch path (bench, batch sweep).  n_frames frames of the same
 * HxW share one subsampling/prefilter setting; params[i] gives frame i's table.
 * Buffers are device pointers: rgb (n*H*W*3 u8), rgb_out (same), coeffs
 * (n * coeffs_per_frame int16, reference layout: Y blocks, Cb blocks, Cr blocks,
 * raster order, each block row-major), stats (n entries, overwritten), each
 * 16-byte aligned (JDS_EINVAL otherwise; hipMalloc / torch allocations are).
 * stream: a hipStream_t (NULL = the HIP null stream).  Asynchronous. */
int jds_plan_create(jds_ctx* ctx, const jds_params* params, int n_frames, int64_t H, int64_t W,
                    jds_plan** out);
/* Quality-sweep plan (BASELINE configs[3]; gui/worker.py:39-74 runs one
 * compress_reconstruct per quality): n_frames frames x n_q tables, params has
 * n_frames * n_q entries, item = frame * n_q + q.  jds_plan_run then takes rgb
 * with n_frames frames and writes rgb_out / coeffs / stats for the n_frames *
 * n_q items.  The quality-independent front end (colour, prefilter, subsample,
 * DCT) runs once per frame and is quantised for every table.
 * 8x8 blocks, n_q <= 8.  jds_plan_create(.., n, ..) = jds_plan_create_q(.., n, 1, ..). */
int jds_plan_create_q(jds_ctx* ctx, const jds_params* params, int n_frames, int n_q, int64_t H, int64_t W,
                      jds_plan** out);
int jds_plan_run(jds_plan* plan, const uint8_t* rgb, uint8_t* rgb_out, int16_t* coeffs,
                 jds_frame_stats* stats, uint32_t flags, void* stream);
int jds_plan_geometry(const jds_plan* plan, jds_geometry* out);
/* Entries the last run's fix-up lists received: [0] forward blocks recomputed exactly (k_fix_fwd),
   [1] inverse tiles the certified fast inverse handed to the exact kernel (k_inv2_list).  A run of
   both phases in one call certifies against the fixed bound |q Q| <= 1152, an inverse-only run
   (JDS_RUN_INV) against the bound it tracks over the tile (max |q| times max Q: larger on most tables, smaller
   where the coefficients are small): [1] of the two can differ, the bytes cannot.
   [1] depends on the plan's earlier runs, the bytes never do.  On the 8x8 4:2:0 / 4:2:2 kernel an
   item whose previous fast inverse recomputed more than 1/8 of its tiles (count * 8 > tiles) runs the
   exact tile code directly: it contributes all of its tiles to [1], whatever this run's content, and
   carries its count forward.  Only a probe run (the 16th, 32nd, ... fast inverse of the plan) and a
   JDS_RUN_INV_FIXALL run measure such an item again; it leaves exact mode when the fresh count is at
   most 1/8 of its tiles.  Coarse items (DC quantiser > 60) of a plan that also has finer tables start
   in exact mode, so they add all their tiles to [1] on every run but the probes.  The 4:4:4 kernel
   (units: waves of 8 blocks) and the 16x16 kernel have no exact mode.  Runs whose inverse is an exact
   kernel (JDS_RUN_EXACT, JDS_RUN_EXACT_INV, JDS_RUN_SSE at 4:4:4 or 16x16, all-coarse 4:2:x plans without
   JDS_RUN_INV_FAST) report [1] = 0 and count neither towards the probe rhythm nor as a previous run;
   a forward-only run leaves [1] as the last inverse left it.  [0] is that of the last certified
   forward (16x16: 0 after a JDS_RUN_EXACT forward). */
int jds_plan_fix_counts(const jds_plan* plan, uint32_t* counts);
void jds_plan_destroy(jds_plan* plan);

/* Launch-level timing of jds_plan_run itself (bench.py's roofline; no reference
 * counterpart -- the reference's Timer covers only the colour conversions,
 * utils/metrics.py:31-48).  While profiling is on, every run of the plan marks
 * its stream before its first launch and after each kernel launch with an event;
 * jds_plan_profile_read waits for the last mark and returns, per kernel name (in
 * first-seen order), the summed time between the mark before it and its own
 * mark, and the number of launches.  "(between runs)" is the time from one run's
 * last mark to the next run's first (host gaps).  The intervals tile the span
 * from the first mark to the last, so their sum equals *span_ms.  Reading resets
 * the record; jds_plan_profile(plan, 0) stops marking.  The event pool holds
 * 8192 marks (~7 per run): a read after more marks than that fails with
 * JDS_EINVAL ("profile overflow") and returns no totals. */
typedef struct {
  char name[64];
  double total_ms;
  int64_t launches;
} jds_kernel_time;
int jds_plan_profile(jds_plan* plan, int enable);
int jds_plan_profile_read(jds_plan* plan, jds_kernel_time* out, int max, int* n_out, double* span_ms);
/* The same marks for the batch calls of a context (jds_jpeg_batch_to_rgb): the
 * kernels by name, "(batch upload)" (the one host-to-device copy and the
 * zero-fills), "(batch download)", "(between calls)".  The first k_dec_sync of a
 * call includes the descriptors' upload, and every one the host read of the
 * round before it. */
int jds_ctx_profile(jds_ctx* ctx, int enable);
int jds_ctx_profile_read(jds_ctx* ctx, jds_kernel_time* out, int max, int* n_out, double* span_ms);

/* Host-buffer path: the drop-in for engines.pipeline.compress_reconstruct
 * (engines/pipeline.py:17-167).  Synchronous.  rgb: HxWx3 u8, C-contiguous.
 * Outputs (caller-allocated, all but rgb_out/stats nullable):
 *   rgb_out       HxWx3 u8   reconstructed_image            (:95)
 *   coeffs        coeffs_per_frame int16  all_quantized_coeffs (:99)
 *   error_map_y   HxW f64    |Y - Y_rec|                     (:119-120)
 *   error_map_rgb HxW f64    mean_c |rgb - rgb_rec_f|        (:121)
 *   sel           selected luma block (sel_by, sel_bx) arrays (:128-151);
 *                 *sel_valid set to 1 if the index is inside the padded grid. */
int jds_compress_reconstruct(jds_ctx* ctx, const jds_params* p, const uint8_t* rgb, int64_t H,
                             int64_t W, uint8_t* rgb_out, int16_t* coeffs, jds_frame_stats* stats,
                             double* error_map_y, double* error_map_rgb, int32_t sel_by,
                             int32_t sel_bx, jds_selected_block* sel, int32_t* sel_valid);

/* PSNR / SSIM of two HxWx3 uint8 host images on the GPU (utils/metrics.py:9-28):
 * out[0..3] = SSIM of R, G, B, Y; out[4] = MSE of Y; out[5] = MSE of RGB.
 * Bit-identical to skimage + scipy.ndimage + NumPy reductions.  H, W >= 7. */
int jds_psnr_ssim(jds_ctx* ctx, const uint8_t* a, const uint8_t* b, int64_t H, int64_t W, double* out);

/* The same on device-resident images (a_dev, b_dev: HxWx3 uint8 in device
 * memory of ctx's device, e.g. a plan's input frames and outputs), run on the
 * context's stream after a device-wide wait for earlier work; out on the host.
 * Serves the batch sweep's per-item CompressionResult metrics
 * (gui/worker.py:62-68 -> utils/metrics.py:9-28) without host copies
 * (SURVEY.md section 5 interface sketch: jds_ssim_dev). */
int jds_psnr_ssim_dev(jds_ctx* ctx, const uint8_t* a_dev, const uint8_t* b_dev, int64_t H, int64_t W, double* out);

/* jds_psnr_ssim_dev without the device-wide wait: the context's stream waits
 * only for the work queued so far on `after` (a hipStream_t, e.g. the plan
 * run's stream; NULL = the HIP null stream; JDS_AFTER_NONE = the caller has
 * already synchronised the images), so leased contexts of other threads keep
 * running.  out on the host. */
int jds_psnr_ssim_dev_after(jds_ctx* ctx, const uint8_t* a_dev, const uint8_t* b_dev, int64_t H, int64_t W,
                            double* out, void* after);

/* The same for n device-resident image pairs of one size (the batch sweep's
 * items, gui/worker.py:62-68): pair i = (a_dev[i], b_dev[i]) (host arrays of
 * device pointers); out[6 i + 0..5] as above.  The pairs run together (from
 * 32 pairs, R, G, B in one launch for all of them; the luma in groups sized by
 * a 16 GB scratch budget), so a sweep's SSIM fills the chip.  `after` as above. */
int jds_psnr_ssim_batch_dev(jds_ctx* ctx, int32_t n, const uint8_t* const* a_dev, const uint8_t* const* b_dev,
                            int64_t H, int64_t W, double* out, void* after);

/* NumPy's float32 sum of magnitude_bits over device-resident int16
 * coefficients (utils/metrics.py:77-78: np.sum(np.ceil(np.log2(|q| + 1)) + 1)
 * over the nonzero q, float32 accumulation in NumPy's 8192-element buffered
 * pairwise order; the host path's k_mag_f32 chain): what bpp and
 * compression_ratio are computed from once the exact sum passes 2^24.
 * n_coeffs: a multiple of 64 (one frame's IntermediateData layout); `after` as
 * above.  *out on the host. */
int jds_magnitude_bits_f32_dev(jds_ctx* ctx, const int16_t* coeffs_dev, int64_t n_coeffs, double* out, void* after);
/* The same for n_items coefficient arrays at coeffs_dev + i * item_stride
 * (int16 elements), one wait: out[i] on the host. */
int jds_magnitude_bits_f32_batch_dev(jds_ctx* ctx, const int16_t* coeffs_dev, int32_t n_items, int64_t n_coeffs,
                                     int64_t item_stride, double* out, void* after);

/* Per-stage functions of the engines.* API (engines/__init__.py:10-27), on host
 * fp64 arrays staged through the context's device memory.  Synchronous.
 *   rgb_to_ycbcr / ycbcr_to_rgb: n_pixels x 3 (engines/color_space.py:8-24)
 *   subsample: cb, cr HxW -> (H/2 or H) x W/2; mode JDS_SS_422 / JDS_SS_420;
 *              gauss = 3 prefilter taps (engines/color_space.py:27-53)
 *   upsample : h x w -> H x W, bilinear (nearest != 0: INTER_NEAREST) (:56-66)
 *   block_dct: n 8x8 blocks; op 0 dct2, 1 idct2, 2 encode_block, 3 decode_block
 *              (engines/dct_engine.py:7-27)
 *   quantize : n values (n % 64 == 0, 8x8-periodic table); dequant = 0:
 *              f64 -> int16 round-half-even of c/Q; 1: int16 -> f64 q*Q
 *              (engines/quantizer.py:22-29) */
int jds_stage_rgb_to_ycbcr(jds_ctx* ctx, const double* rgb, double* ycc, int64_t n_pixels);
int jds_stage_ycbcr_to_rgb(jds_ctx* ctx, const double* ycc, double* rgb, int64_t n_pixels);
int jds_stage_subsample(jds_ctx* ctx, const double* cb, const double* cr, int64_t H, int64_t W, int32_t mode,
                        int32_t prefilter, const double* gauss, double* cb_out, double* cr_out);
int jds_stage_upsample(jds_ctx* ctx, const double* in, int64_t h, int64_t w, int64_t H, int64_t W,
                       int32_t nearest, double* out);
int jds_stage_block_dct(jds_ctx* ctx, const double* in, double* out, int64_t n_blocks, int32_t op);
int jds_stage_quantize(jds_ctx* ctx, const void* in, const double* qtable, void* out, int64_t n,
                       int32_t dequant);
/* The same for 8x8 or 16x16 blocks (block_size 8 / 16; dctn / idctn of a 16x16
 * block, dct_engine.py:7-27) and for a 64- or 256-entry table broadcast over
 * n values (quantizer.py:22-29 with a 16x16 table). */
int jds_stage_block_dct_n(jds_ctx* ctx, const double* in, double* out, int64_t n_blocks, int32_t block_size,
                          int32_t op);
int jds_stage_quantize_n(jds_ctx* ctx, const void* in, const double* qtable, int32_t table_len, void* out,
                         int64_t n, int32_t dequant);

/* Baseline JPEG entropy coding (the reference only estimates
 * the size, utils/metrics.py:51-92): coefficients in the reference's layout
 * (all_quantized_coeffs, engines/pipeline.py:56,99) -> one JFIF file per frame:
 * SOI, APP0, DQT (the frame's 8x8 table, zigzag order, utils/constants.py:18-27),
 * SOF0, the T.81 Annex K Huffman tables, three non-interleaved scans (Y, Cb, Cr),
 * EOI.  Byte-for-byte definition: oracle/jpeg_entropy.py.  8x8 blocks only;
 * tables must hold integers in [1, 255].
 *   jds_plan_entropy: device buffers; coeffs as jds_plan_run writes them; frame i's
 *     file at out + i*out_stride (out_stride >= jds_plan_entropy_capacity), its
 *     length in lengths[i] (u64, device), and optionally the entropy-coded bits of
 *     its Y/Cb/Cr scans in scan_bits[3*i..] (before the byte pad).  Asynchronous.
 *     lengths[i] = 0 marks a frame whose coefficients baseline JPEG cannot code
 *     (DC difference category > 11 or AC category > 10; the codec path never
 *     produces those).
 *   jds_encode_jfif: one frame from host memory (synchronous); *out_len is set even
 *     when out_cap is too small (then JDS_EINVAL). */
int jds_plan_entropy_capacity(const jds_plan* plan, int64_t* bytes_per_frame);
int jds_plan_entropy(jds_plan* plan, const int16_t* coeffs, uint8_t* out, int64_t out_stride, uint64_t* lengths,
                     uint64_t* scan_bits, void* stream);
int jds_encode_jfif(jds_ctx* ctx, const jds_params* p, int64_t H, int64_t W, const int16_t* coeffs, uint8_t* out,
                    int64_t out_cap, int64_t* out_len, uint64_t* scan_bits);

/* Baseline JFIF decoding (DESIGN.md "Entropy decode"): the files this library
 * writes -- and any baseline file of the same profile -- back to
 * all_quantized_coeffs (reference layout) and on to the RGB image.
 *
 * Profile: SOF0, 8-bit, components 1, 2, 3, Y sampled 1x1 / 2x1 / 2x2 with 1x1
 * chroma, one quantisation table, three non-interleaved scans in any order,
 * Huffman tables from the file's DHT segments; APPn / COM are skipped.
 * Restart intervals (T.81 B.2.4.4, E.1.4): a DRI segment (length 4, else
 * JDS_EINVAL) sets the interval Ri for the scans that follow, Ri = 0 switches
 * restarts off, DRI may appear more than once.  A non-interleaved scan's MCU is
 * one block, so a scan of nb blocks then holds ceil(nb / Ri) - 1 markers, the
 * i-th being RST(i & 7); a wrong count or order is JDS_EINVAL (the message names
 * the scan and DRI), as is an RSTm with Ri = 0 or outside scan data.  Fill
 * bytes (FF FF) before a marker inside such a scan are JDS_ENOTSUP.
 * Anything else in a well-formed file is JDS_ENOTSUP (the message names the
 * feature), malformed bytes are JDS_EINVAL; sizes whose T.81 chroma block grid
 * differs from the reference's floor-sized planes are JDS_ENOTSUP as for the
 * encoder.
 *
 * The entropy decode is self-synchronising: every scan is cut into
 * subsequences of a fixed number of bits, one GPU lane decodes each from a
 * guessed state, and exit states are handed to the next subsequence until none
 * changes -- inside a workgroup in one launch, across workgroups between
 * launches (the host reads a counter after each round).  A scan with restart
 * intervals needs none of that: every interval is a stream of its own whose
 * first block is known, one lane decodes it in one pass (0 rounds).  A frame's
 * status word is 0 or a combination of JDS_DEC_* bits. */
#define JDS_DEC_HEADER   1u  /* plan path: header differs from the plan's, or lengths[i] == 0 */
#define JDS_DEC_CODE     2u  /* invalid Huffman code (or a size outside baseline) */
#define JDS_DEC_K63      4u  /* a run past coefficient 63 */
#define JDS_DEC_OVERRUN  8u  /* the scan data end inside a symbol */
#define JDS_DEC_COUNT    16u /* the scan holds fewer or more blocks than the frame needs */
#define JDS_DEC_DC_RANGE 32u /* a DC value (sum of the differences) outside int16 */
#define JDS_DEC_RESTART  64u /* the restart markers are not the ones the geometry and the interval require */

typedef struct {
  int32_t component;          /* 1 Y, 2 Cb, 3 Cr */
  int32_t dc_table, ac_table; /* Huffman table ids (0 / 1) */
  int32_t restart_interval;   /* the DRI interval in effect at this scan's SOS (MCUs = blocks), 0: none */
  int64_t offset, length;     /* the entropy-coded segment: stuffed bytes up to the next marker, RSTm markers included */
} jds_jfif_scan;

typedef struct {
  uint8_t bits[16];  /* BITS: codes per length 1..16 */
  uint8_t vals[256]; /* HUFFVAL */
  int32_t n_vals;
  int32_t defined;
} jds_jfif_huff;

typedef struct {
  int64_t H, W;
  int32_t subsampling;      /* JDS_SS_* */
  int32_t n_scans;          /* 3 */
  double qtable[64];        /* row-major (de-zigzagged), as jds_params.qtable */
  jds_jfif_scan scan[3];    /* in file order */
  jds_jfif_huff huff[4];    /* [0] DC 0, [1] DC 1, [2] AC 0, [3] AC 1, from the file's DHT segments */
  int64_t y_blocks, c_blocks; /* blocks of the Y scan / of each chroma scan */
  int64_t coeffs_needed;    /* int16 entries of the coefficient buffer: 64 * (y_blocks + 2 * c_blocks) */
  uint32_t status;          /* jds_decode_jfif / jds_decompress_jfif: the frame's JDS_DEC_* bits */
  uint32_t rounds;          /* the same calls: inter-workgroup propagation rounds */
} jds_jfif_info;

/* Host only, no device access (like jds_geometry_of); never reads outside [data, data + len). */
int jds_jfif_parse(const uint8_t* data, int64_t len, jds_jfif_info* out);
/* One file from host memory to host coefficients (synchronous).  *info is
 * filled even when coeffs_cap (int16 entries) is too small (then JDS_EINVAL;
 * info->coeffs_needed holds the need).  A non-zero frame status is JDS_EINVAL
 * with a message naming the defect. */
int jds_decode_jfif(jds_ctx* ctx, const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap,
                    jds_jfif_info* info);
/* Decode, then the plan's default inverse for the file's geometry and table
 * (an inverse-only jds_plan_run on zeroed statistics): rgb_out (H*W*3 bytes,
 * rgb_cap >= that) is this codec's reconstruction of the coefficients, the
 * bytes jds_compress_reconstruct returned as rgb_out for the frame that made
 * the file.  coeffs: NULL, or info->coeffs_needed int16 entries (see
 * jds_jfif_parse). */
int jds_decompress_jfif(jds_ctx* ctx, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                        int16_t* coeffs, jds_jfif_info* info);
/* Device-resident batch decode, the mirror of jds_plan_entropy: frame i's file
 * at files + i*stride with lengths[i] bytes (u64, device), its coefficients to
 * coeffs + i*coeffs_per_frame, its status word to status[i] (u32, device).
 * Each header is compared on the device with the one the plan writes; a
 * mismatch or lengths[i] == 0 sets JDS_DEC_HEADER and skips the frame (its
 * coefficients are zero).  Scan offsets come from a marker search on the
 * device; all frames and scans decode in the same launches.  NOT asynchronous:
 * the call waits for `stream` after the header pass and after every
 * propagation round, and returns with the coefficients queued on `stream`.  A
 * following jds_plan_run(.., JDS_RUN_INV) reconstructs; on a plan that never
 * ran its forward, give it zeroed stats: afterwards they hold total_coeffs,
 * block_overhead_bits and pixels, everything else as given. */
int jds_plan_entropy_decode(jds_plan* plan, const uint8_t* files, int64_t stride, const uint64_t* lengths,
                            int16_t* coeffs, uint32_t* status, void* stream);
/* The decoder's compile-time constants: bits per subsequence, subsequences per workgroup. */
int jds_entropy_decode_info(int32_t* subseq_bits, int32_t* subseq_per_group);
/* Inter-workgroup propagation rounds (launches of the synchronisation kernel) the plan's last decode took. */
int jds_plan_entropy_decode_rounds(const jds_plan* plan, uint32_t* rounds);

/* Restart intervals (DESIGN.md "Restart intervals").  The writer codes in
 * independent 64-block segments, one wave each; with interval 64 every segment
 * is a restart interval: DRI after the last DHT, every interval padded to its
 * byte, RST(i - 1 & 7) in front of interval i >= 1 of a scan.  Byte-for-byte
 * definition: tests/restart_ref.py over oracle/jpeg_entropy.py.
 *   jds_entropy_restart_info: the one interval the writer supports besides 0
 *     (64), and the largest interval the decoder gives to one lane (files with a
 *     larger one decode through the self-synchronising kernels, one descriptor
 *     per interval).
 *   The _rst calls mirror their plain namesakes; interval 0 is JDS_EINVAL (the
 *     plain calls write plain files), any value but the writer's is JDS_ENOTSUP.
 *   jds_plan_entropy_decode_rst: as jds_plan_entropy_decode for the files
 *     jds_plan_entropy_rst writes, but ASYNCHRONOUS: the plan knows every
 *     frame's marker count, so nothing is read back.  A frame whose markers
 *     (SOS, RST0, RST1, .., SOS, .., EOI) are not the ones its geometry and the
 *     interval require gets JDS_DEC_RESTART and, like a JDS_DEC_HEADER frame,
 *     zero coefficients.  The interval must not exceed lane_max_blocks. */
int jds_entropy_restart_info(int32_t* writer_interval, int32_t* lane_max_blocks);
int jds_plan_entropy_capacity_rst(const jds_plan* plan, int32_t interval, int64_t* bytes_per_frame);
int jds_plan_entropy_rst(jds_plan* plan, int32_t interval, const int16_t* coeffs, uint8_t* out, int64_t out_stride,
                         uint64_t* lengths, uint64_t* scan_bits, void* stream);
int jds_encode_jfif_rst(jds_ctx* ctx, const jds_params* p, int64_t H, int64_t W, int32_t interval,
                        const int16_t* coeffs, uint8_t* out, int64_t out_cap, int64_t* out_len, uint64_t* scan_bits);
int jds_plan_entropy_decode_rst(jds_plan* plan, int32_t interval, const uint8_t* files, int64_t stride,
                                const uint64_t* lengths, int16_t* coeffs, uint32_t* status, void* stream);

/* Optimised Huffman tables (DESIGN.md "Optimised tables"): each frame is coded
 * with its own four tables, built from the frame's symbol counts (libjpeg
 * -optimize, Pillow optimize=True).  Byte-for-byte definition:
 * tests/huffopt_ref.py over oracle/jpeg_entropy.py.  The file holds SOI, APP0,
 * DQT, SOF0 as the standard route writes them, four DHT segments (0x00, 0x10,
 * 0x01, 0x11) that list only the symbols the frame uses, DRI for a restart
 * file, and the three scans.  Luma tables count the Y scan, chroma tables the
 * Cb and Cr scans together; with a restart interval the DC differences restart
 * at every interval, so the two file forms have different tables.  The tables
 * are T.81 K.2 with libjpeg's tie rules and K.3; a class whose codes would
 * exceed 32 bits before K.3 (about 15 million symbols) keeps its Annex K table.
 *   interval: 0, or the writer's (jds_entropy_restart_info); anything else is
 *     JDS_ENOTSUP.
 *   jds_plan_entropy_capacity_opt: the route's own worst case.  Any symbol may
 *     get a 16-bit code, so a block is bounded by 1665 bits instead of 1660 and
 *     the bound is larger than jds_plan_entropy_capacity[_rst]'s.
 *   jds_plan_entropy_opt: as jds_plan_entropy[_rst]; ASYNCHRONOUS -- counts,
 *     tables, headers and files are made on the device, nothing is read back.
 *     lengths[i] == 0 keeps its meaning (a frame baseline JPEG cannot code).
 *   jds_encode_jfif_opt: as jds_encode_jfif[_rst].
 * Reading: jds_decode_jfif, jds_decompress_jfif, jds_decode_jpeg and
 * jds_jpeg_batch_to_rgb take the files (they read each file's DHT).
 * jds_plan_entropy_decode[_rst] compare headers with the plan's own and mark
 * optimised files JDS_DEC_HEADER. */
int jds_plan_entropy_capacity_opt(const jds_plan* plan, int32_t interval, int64_t* bytes_per_frame);
int jds_plan_entropy_opt(jds_plan* plan, int32_t interval, const int16_t* coeffs, uint8_t* out, int64_t out_stride,
                         uint64_t* lengths, uint64_t* scan_bits, void* stream);
int jds_encode_jfif_opt(jds_ctx* ctx, const jds_params* p, int64_t H, int64_t W, int32_t interval,
                        const int16_t* coeffs, uint8_t* out, int64_t out_cap, int64_t* out_len, uint64_t* scan_bits);
/* Test-only.  jds_selftest_huffopt (host, no GPU): the table of freq[0..255] by
 * the core the kernel shares (csrc/jds_huffopt.hpp): BITS[1..16], HUFFVAL (256
 * bytes, n_vals used), fell_back = 1 when a code would exceed 32 bits, in which
 * case the Annex K AC luma table is returned.  jds_selftest_huffopt_dev: the
 * same fields from k_ent_opt_tables for n histograms (freqs: n x 256 counts,
 * bits_out n x 16, vals_out n x 256, n_vals and fell_back n each; host
 * pointers). */
int jds_selftest_huffopt(const uint32_t* freq, uint8_t* bits_out, uint8_t* vals_out, int32_t* n_vals,
                         int32_t* fell_back);
int jds_selftest_huffopt_dev(jds_ctx* ctx, const uint32_t* freqs, int32_t n, uint8_t* bits_out, uint8_t* vals_out,
                             int32_t* n_vals, int32_t* fell_back);

/* Baseline JPEGs from elsewhere (DESIGN.md "Interleaved scans").  The calls
 * above read the profile this library writes; libjpeg, Pillow, cameras and
 * browsers write another: ONE interleaved scan (Ns = 3, MCUs of Y.. Cb Cr
 * blocks) and a quantisation table per component.  jds_jpeg_parse accepts
 * everything jds_jfif_parse accepts and in addition
 *   - one scan with Ns = 3 (components 1, 2, 3 in that order) instead of three
 *     with Ns = 1; Ns = 2 and a mix of the two forms are JDS_ENOTSUP;
 *   - up to three 8-bit quantisation tables, Tq per component;
 *   - T.81's block grids at every size: component c has
 *     ceil(ceil(W * Hc / Hmax) / 8) columns (rows alike); reference_grid says
 *     whether they equal the floor-sized grids of the calls above;
 *   - with an interleaved scan DRI counts MCUs: ceil(nMCU / Ri) - 1 markers,
 *     RST0, RST1, .. in order;
 *   - grayscale files (DESIGN.md "Grayscale files"): SOF0 with Nf = 1, any
 *     component id 0..255 (the SOS must name the same one), sampling factors
 *     1..4 each -- which are then IGNORED: a one-component scan is never
 *     interleaved (T.81 A.2.2), so the block grid is ceil(W/8) x ceil(H/8)
 *     whatever the byte says (Pillow writes 0x22 with subsampling=2; libjpeg
 *     reads such files as 1x1) -- and exactly one scan with Ns = 1, whose DRI
 *     counts blocks.  subsampling = JDS_SS_GRAY, n_scans = 1, interleaved = 0,
 *     blocks_per_mcu = 1, hs[0] = vs[0] = 1, mcu_cols / mcu_rows = the grid,
 *     single_table = 1, reference_grid = 0; hs, vs, tq, grid_cols, grid_rows and
 *     qtable of components 1 and 2 are zero; scan[0].component[0] is 1 (the
 *     file's own id stays in its header).  A scan with Ns != 1, a scan naming
 *     another id, or a second scan in such a frame is an error naming
 *     "grayscale".
 * Still rejected by name: progressive, arithmetic, 12-bit, two- and
 * four-component frames (CMYK / YCCK), 16-bit DQT, Huffman ids above 1, DHT
 * redefined between scans, component ids other than 1, 2, 3 in a
 * three-component frame, luma sampling other than 1x1, 2x1, 2x2, subsampled
 * chroma.  jds_jfif_parse keeps this library's own profile and rejects
 * grayscale files.
 *
 * Coefficient layout of every decode: Y, Cb, Cr planar, each component's
 * blocks in raster order of its T.81 grid, each block row-major (a grayscale
 * file: the one plane);
 * coeffs_needed = 64 * sum of the grid sizes (with reference_grid set: exactly
 * the layout of jds_decode_jfif).  The blocks an interleaved scan carries
 * beyond the grids (padding to whole MCUs) are decoded, count in their
 * component's DC prediction and are dropped. */
typedef struct {
  int32_t n_components;       /* Ns: 3 (interleaved) or 1 */
  int32_t component[3];       /* 1 Y, 2 Cb, 3 Cr, in scan order (a grayscale file's component: 1) */
  int32_t dc_table[3], ac_table[3]; /* Huffman table ids (0 / 1) per scan component */
  int32_t restart_interval;   /* DRI in effect at SOS, in MCUs of this scan (Ns = 1: blocks); 0: none */
  int64_t offset, length;     /* the entropy-coded segment, RSTm markers included */
} jds_jpeg_scan;

typedef struct {
  int64_t H, W;
  int32_t subsampling;        /* JDS_SS_*; JDS_SS_GRAY: one component */
  int32_t n_scans;            /* 1 (interleaved, or grayscale) or 3 */
  int32_t interleaved;        /* 1: one scan with Ns = 3 */
  int32_t reference_grid;     /* 1: the T.81 grids are the ones jds_jfif_parse accepts */
  int32_t single_table;       /* 1: one quantisation table serves all three components */
  int32_t blocks_per_mcu;     /* of the interleaved MCU: 6 (4:2:0), 4 (4:2:2), 3 (4:4:4); grayscale: 1 */
  int32_t hs[3], vs[3];       /* sampling factors per component (grayscale: 1 x 1, zero for the absent ones) */
  int32_t tq[3];              /* quantisation table id per component */
  int64_t mcu_cols, mcu_rows; /* ceil(W / (8 Hmax)), ceil(H / (8 Vmax)) */
  int64_t grid_cols[3], grid_rows[3]; /* T.81 block grid per component (zero for an absent one) */
  double qtable[3][64];       /* per component, row-major (de-zigzagged; zero for an absent one) */
  jds_jpeg_scan scan[3];      /* in file order */
  jds_jfif_huff huff[4];      /* [0] DC 0, [1] DC 1, [2] AC 0, [3] AC 1 */
  int64_t coeffs_needed;      /* 64 * sum of grid_cols[c] * grid_rows[c] */
  uint32_t status;            /* jds_decode_jpeg: the frame's JDS_DEC_* bits */
  uint32_t rounds;            /* jds_decode_jpeg: inter-workgroup propagation rounds */
} jds_jpeg_info;

/* Host only, no device access; never reads outside [data, data + len). */
int jds_jpeg_parse(const uint8_t* data, int64_t len, jds_jpeg_info* out);
/* One file from host memory to host coefficients (synchronous); the error
 * contract of jds_decode_jfif.  An interleaved scan decodes through the
 * interleaved instantiations of the same kernels: the decoder state carries
 * the block's slot in the MCU, the tables are chosen per slot, DC differences
 * go to a scan-order staging array and a per-component segmented sum places the
 * values.  Restart intervals of at most lane_max_blocks blocks
 * (Ri * blocks_per_mcu) decode one per lane, longer ones one descriptor each. */
int jds_decode_jpeg(jds_ctx* ctx, const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap,
                    jds_jpeg_info* info);
/* jds_decompress_jfif for a file of either scan form that the plan's inverse can
 * take: one quantisation table for all components (single_table) and the
 * reference's block grids (reference_grid); anything else is JDS_ENOTSUP.  Such
 * files -- a table per component, other grids, grayscale -- are reconstructed stage by
 * stage with the file's own tables (jds.codec.decompress_jpeg: jds_stage_quantize_n,
 * jds_stage_block_dct_n, jds_stage_upsample, jds_stage_ycbcr_to_rgb), not a
 * throughput path.  coeffs: NULL, or info->coeffs_needed entries. */
int jds_decompress_jpeg(jds_ctx* ctx, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                        int16_t* coeffs, jds_jpeg_info* info);
/* Foreign files to pixels (DESIGN.md "Foreign files to pixels"): the fused
 * inverse k_jpeg_inv takes the coefficients of jds_decode_jpeg (any file
 * jds_jpeg_parse accepts: either scan form, a table per component, T.81 grids at
 * any size) to RGB bytes in one launch, byte for byte what the per-stage route
 * (jds.codec.staged_inverse) reconstructs: dequantise with the component's
 * table, the exact fp64 IDCT, +128, clip, crop chroma to its T.81 plane
 * ceil(H Vc / Vmax) x ceil(W Hc / Hmax), cv2 INTER_LINEAR with its general taps
 * to H x W, NumPy's colour expressions, clip, truncate.  A grayscale file
 * (JDS_SS_GRAY) gives (Y, Y, Y) per pixel -- the same definition at neutral
 * chroma, where the colour expressions are Y + c * 0.0 = Y -- through an
 * instantiation of its own that reads the one plane and the one table only:
 * qtable, grid_rows / grid_cols of component 0 and coeffs_needed = one plane are
 * checked, the rest of info is not read.
 *
 * jds_jpeg_inverse_info: the tile of output pixels one workgroup produces
 *   (compile-time constants, multiples of 16).
 * jds_jpeg_inverse_dev: coeffs (info->coeffs_needed int16) and rgb (H*W*3
 *   bytes) are device pointers of the context's device; one launch on `stream`,
 *   asynchronous, nothing uploaded or read back (the tables travel as kernel
 *   arguments).  Reads H, W, subsampling, grid_rows/cols, coeffs_needed and
 *   qtable of info; a table entry outside integer [1, 255] or grids other than
 *   T.81's for H x W are JDS_EINVAL (checked before anything else).
 * jds_jpeg_to_rgb: parse, decode and that launch on the context's stream, then
 *   the image into rgb_out: host memory, or with rgb_on_device != 0 a device
 *   buffer of the context's device (written in place by the kernel).
 *   Synchronous either way.  Here and at every *_on_device parameter of this
 *   header the context's stream waits for no other stream: a device buffer
 *   must be idle, or the work queued on it ordered before the call.
 *   coeffs: NULL, or host memory of coeffs_needed
 *   entries.  The error contract of jds_decode_jpeg; on a defective scan
 *   (JDS_EINVAL naming the defect) rgb_out is not written and the context stays
 *   usable. */
int jds_jpeg_inverse_info(int32_t* tile_h, int32_t* tile_w);
int jds_jpeg_inverse_dev(jds_ctx* ctx, const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb, void* stream);
int jds_jpeg_to_rgb(jds_ctx* ctx, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                    int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_info* info);
/* Test-only, host-only: the kernel's tile core (csrc/jds_jpeg_inv.hpp) in a
 * host tile loop with the same window function; the argument checks of
 * jds_jpeg_inverse_dev.  No GPU. */
int jds_selftest_jpeg_inverse(const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb_out);
/* Test-only: jpeg_inv_window on one axis: the chroma samples [out[0], out[0] +
 * out[1]) that destination indices d0..d1 of a dst_n-long axis read from a
 * src_n-long one (xaxis: cv2's clamped column taps); out[2], out[3]: the rows
 * and columns the kernel's window array holds on a subsampled axis. */
int jds_selftest_jpeg_window(int32_t d0, int32_t d1, int32_t dst_n, int32_t src_n, int32_t xaxis, int32_t* out);
/* Test-only: jds_decode_jpeg's algorithm on the host (see jds_selftest_huffdec).
 * rounds_out[3]: decode rounds per scan in file order (an interleaved file has
 * one scan; 0 for a scan with restart intervals).  No GPU. */
int jds_selftest_jpegdec(const uint8_t* data, int64_t len, int32_t subseq_bits, int16_t* coeffs, int64_t coeffs_cap,
                         int32_t* rounds_out);

/* Batches of foreign files (DESIGN.md "Batches of foreign files"): n files of
 * any mix of sizes, subsampling modes, tables, restart intervals and scan forms
 * through ONE set of launches -- the entropy decode over the descriptors of
 * every file (as many propagation rounds as the slowest file needs), then
 * k_jpeg_inv_batch once per mode present (4:4:4, 4:2:2, 4:2:0, grayscale; a
 * grayscale item's subsampling is JDS_SS_GRAY and its image H x W x 3 like the
 * others') -- into one output buffer.
 *
 * Layout: file i's image starts at items[i].rgb_off, a multiple of 256, and the
 *   images follow one another in batch order; rgb_bytes is the sum of the
 *   images' sizes, each rounded up to 256.  The bytes between an image's end
 *   and the next multiple of 256 are never written.  Its coefficients
 *   (jds_decode_jpeg's layout) are entries [coef_off, coef_off + coeffs_needed)
 *   of the batch's coefficient buffer, end to end; coef_entries is their sum.
 * A file jds_jpeg_parse rejects, or whose tables or geometry the checks of
 *   jds_jpeg_inverse_dev refuse, is an ITEM error: items[i].rc carries the code
 *   that call gives for the file alone, the file takes no space (rgb_off and
 *   coef_off -1, coeffs_needed 0) and the batch goes on.  The call then still
 *   returns JDS_OK, and jds_last_error names the first such file by index
 *   ("file 3: ...").
 * A file whose SCAN DATA are defective keeps its space: items[i].status carries
 *   the JDS_DEC_* bits jds_decode_jpeg reports for it, its pixels are all zero
 *   (the inverse reads the status word on the device), its coefficients are
 *   unspecified, and no other file's bytes are affected.
 * jds_jpeg_batch_layout: host only; parse every file, lay the outputs out.
 * jds_jpeg_batch_to_rgb: synchronous.  rgb: rgb_cap >= rgb_bytes bytes of host
 *   memory, or with rgb_on_device != 0 of the context's device (the images are
 *   written in place and only the status words come back).  coeffs: NULL, or
 *   host memory of coef_entries entries.  rounds (nullable): the propagation
 *   rounds of the batch, the largest any of its files needs.  n == 0 is valid.
 *   The file bytes are gathered into one pinned staging buffer of the context
 *   (each file at a 16-byte boundary) and uploaded once together with the
 *   descriptors, table sets, MCU and inverse records.  JDS_ENOTSUP: more blocks,
 *   tiles or intervals than the grids and 32-bit indices take.
 * jds_selftest_jpeg_batch: test-only, host only: the same layout, the host
 *   decode model per file (jds_selftest_jpegdec) and the host model of the batch
 *   inverse (the same tile map and per-image records).  coeffs may be NULL. */
typedef struct {
  int32_t rc;        /* JDS_OK, or the code jds_jpeg_parse / the inverse's checks gave this file */
  uint32_t status;   /* JDS_DEC_* bits of its scan data; 0: decoded */
  int64_t H, W;
  int32_t subsampling, interleaved;
  int64_t rgb_off;   /* its image's first byte in the output; a multiple of 256 */
  int64_t coef_off;  /* its first coefficient in the batch's coefficient buffer */
  int64_t coeffs_needed;
} jds_jpeg_batch_item;
int jds_jpeg_batch_layout(const uint8_t* const* data, const int64_t* lens, int32_t n, jds_jpeg_batch_item* items,
                          int64_t* rgb_bytes, int64_t* coef_entries);
int jds_jpeg_batch_to_rgb(jds_ctx* ctx, const uint8_t* const* data, const int64_t* lens, int32_t n, uint8_t* rgb,
                          int64_t rgb_cap, int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items,
                          uint32_t* rounds);
int jds_selftest_jpeg_batch(const uint8_t* const* data, const int64_t* lens, int32_t n, int32_t subseq_bits,
                            uint8_t* rgb, int64_t rgb_cap, int16_t* coeffs, jds_jpeg_batch_item* items);

/* The libjpeg rendering (DESIGN.md "libjpeg rendering"; definition:
 * tests/libjpeg_ref.py): a second rendering of the same decoded coefficients,
 * byte for byte what libjpeg (libjpeg-turbo, hence Pillow, OpenCV, torchvision,
 * browsers) gives with its default settings -- dequantise, the ISLOW integer
 * IDCT (jidctint), +128, clamp, crop chroma to its T.81 plane, fancy upsampling
 * (jdsample's h2v1 / h2v2 triangle taps; replication when the chroma plane is at
 * most two samples wide), jdcolor's 16-bit fixed-point YCbCr -> RGB, clamp.
 * `render` selects: JDS_RENDER_REFERENCE is the rendering above (k_jpeg_inv),
 * and each _render call with it does exactly what its namesake without the
 * argument does; JDS_RENDER_LIBJPEG runs k_jpeg_ljt / k_jpeg_ljt_batch.  Any
 * other value is JDS_EINVAL ("unknown render ...").
 *
 * Scope: parity with libjpeg is stated for files it decodes as YCbCr (JFIF, or
 *   no Adobe marker with ordinary component ids) or as grayscale, and for its
 *   default settings only (ISLOW, fancy upsampling, no block smoothing), at
 *   full size and, through the _scaled calls below, at libjpeg's scales 1/2,
 *   1/4 and 1/8 (its other M/8 scales are not offered).  A file libjpeg would
 *   take as RGB (Adobe transform 0, or ids 'R', 'G', 'B') is still treated as
 *   YCbCr here, as by every other call.
 *   jds_decompress_jpeg, the transcode and the transforms have no rendering
 *   argument.
 * Arithmetic: 32-bit two's complement with wrap-around at every operation.
 *   While every dequantised coefficient (coefficient x table entry) of a block
 *   is within +-1173, or their absolute values sum to at most 14107 over the
 *   block, no intermediate leaves 31 bits (DESIGN.md derives both bounds; blocks
 *   coded from 8-bit samples are of the first kind) and the result is that of
 *   libjpeg-turbo's SIMD decode, which saturates its output as this core does.
 *   libjpeg's C inverse indexes a range table with x & 1023 instead: it gives
 *   the same bytes only where the unclamped sample lies in about [-384, 639].
 *   Beyond the bounds the result is defined -- kernel, host core and
 *   tests/libjpeg_ref.py agree on every int16 input -- but need not be any
 *   libjpeg's.
 *
 * jds_jpeg_render_dev: jds_jpeg_inverse_dev's arguments, checks and contract.
 * jds_jpeg_to_rgb_render, jds_jpeg_batch_to_rgb_render: their namesakes'
 *   arguments and contracts (a batch: zeros for an image with defective scan
 *   data, the bytes between images never written).
 * jds_selftest_jpeg_render, jds_selftest_jpeg_batch_render: test-only, host
 *   only: the tile core (csrc/jds_jpeg_ljt.hpp) in a host tile loop. */
#define JDS_RENDER_REFERENCE 0
#define JDS_RENDER_LIBJPEG 1
int jds_jpeg_render_dev(jds_ctx* ctx, const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb, void* stream,
                        int32_t render);
int jds_jpeg_to_rgb_render(jds_ctx* ctx, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                           int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_info* info, int32_t render);
int jds_jpeg_batch_to_rgb_render(jds_ctx* ctx, const uint8_t* const* data, const int64_t* lens, int32_t n, uint8_t* rgb,
                                 int64_t rgb_cap, int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items,
                                 uint32_t* rounds, int32_t render);
int jds_selftest_jpeg_render(const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb_out, int32_t render);
int jds_selftest_jpeg_batch_render(const uint8_t* const* data, const int64_t* lens, int32_t n, int32_t subseq_bits,
                                   uint8_t* rgb, int64_t rgb_cap, int16_t* coeffs, jds_jpeg_batch_item* items,
                                   int32_t render);

/* The scaled libjpeg rendering (DESIGN.md "Scaled libjpeg rendering";
 * definition: tests/libjpeg_scaled_ref.py): the reduced-size decode libjpeg does
 * inside the IDCT with scale_num / scale_denom = 1 / scale_denom -- Pillow's
 * Image.draft and thumbnail, OpenCV's IMREAD_REDUCED_COLOR_2/4/8 -- byte for
 * byte.  scale_denom is 1, 2, 4 or 8; anything else is JDS_EINVAL naming the
 * value.  1 is the unscaled call: each _scaled call with it does exactly what
 * its _render namesake does.  Another denominator needs JDS_RENDER_LIBJPEG
 * (JDS_EINVAL with JDS_RENDER_REFERENCE: the reference has no scaled decode)
 * and runs k_jpeg_ljs / k_jpeg_ljs_batch.
 *
 * The image is ceil(H / scale_denom) x ceil(W / scale_denom) x 3.  With
 *   m = 8 / scale_denom, luma blocks go through jidctred's m-point inverse
 *   (4 x 4, 2 x 2, 1 x 1); chroma through the s-point one, s being m doubled
 *   while s < 8 and the luma's extent (Hmax m, Vmax m) is a multiple of 2 s --
 *   4:2:0: 8, 4, 2 (one chroma sample per pixel, no upsampling); 4:2:2 and
 *   4:4:4: m.  The chroma plane is cropped to ceil(H s / (8 Vmax)) x
 *   ceil(W s / (8 Hmax)) before the h2v1 upsampling 4:2:2 keeps: fancy taps
 *   when m > 1 and the plane is more than two samples wide, replication
 *   otherwise.  Colour as at full size.  Arithmetic: 32-bit two's complement
 *   with wrap-around; kernel, host core and the definition agree on every
 *   int16 input.
 * jds_jpeg_scaled_size: host only; the image's size at a denominator.
 * jds_jpeg_render_scaled_dev: jds_jpeg_render_dev's
 *   arguments, checks and contract; rgb holds out_h * out_w * 3 bytes.
 * jds_jpeg_to_rgb_scaled: jds_jpeg_to_rgb_render's; rgb_cap >= out_h*out_w*3.
 * jds_jpeg_batch_layout_scaled, jds_jpeg_batch_to_rgb_scaled: scale_denoms
 *   (NULL: all 1) holds one denominator per file, and a batch may mix them.
 *   The layout rule is unchanged with the OUTPUT sizes: images at multiples of
 *   256 in batch order, the bytes between never written, zeros over the scaled
 *   image of a file with defective scan data, item errors stay item errors.
 *   items[i].H / .W stay the file's own; scaled (nullable) receives per file
 *   its denominator and output size.  A bad denominator or a scaled reference
 *   rendering fails the whole call before any work.
 * jds_selftest_jpeg_render_scaled, jds_selftest_jpeg_batch_render_scaled:
 *   test-only, host only: the tile core (csrc/jds_jpeg_ljs.hpp) in a host tile
 *   loop. */
typedef struct {
  int32_t scale_denom, reserved;
  int64_t out_h, out_w; /* ceil(H / scale_denom), ceil(W / scale_denom); 0 for a file with rc != 0 */
} jds_jpeg_scaled_item;
int jds_jpeg_scaled_size(int64_t H, int64_t W, int32_t scale_denom, int64_t* out_h, int64_t* out_w);
int jds_jpeg_render_scaled_dev(jds_ctx* ctx, const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb,
                               void* stream, int32_t render, int32_t scale_denom);
int jds_jpeg_to_rgb_scaled(jds_ctx* ctx, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                           int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_info* info, int32_t render,
                           int32_t scale_denom);
int jds_jpeg_batch_layout_scaled(const uint8_t* const* data, const int64_t* lens, int32_t n,
                                 jds_jpeg_batch_item* items, int64_t* rgb_bytes, int64_t* coef_entries,
                                 const int32_t* scale_denoms, jds_jpeg_scaled_item* scaled);
int jds_jpeg_batch_to_rgb_scaled(jds_ctx* ctx, const uint8_t* const* data, const int64_t* lens, int32_t n,
                                 uint8_t* rgb, int64_t rgb_cap, int32_t rgb_on_device, int16_t* coeffs,
                                 jds_jpeg_batch_item* items, uint32_t* rounds, int32_t render,
                                 const int32_t* scale_denoms, jds_jpeg_scaled_item* scaled);
int jds_selftest_jpeg_render_scaled(const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb_out, int32_t render,
                                    int32_t scale_denom);
int jds_selftest_jpeg_batch_render_scaled(const uint8_t* const* data, const int64_t* lens, int32_t n,
                                          int32_t subseq_bits, uint8_t* rgb, int64_t rgb_cap, int16_t* coeffs,
                                          jds_jpeg_batch_item* items, int32_t render, const int32_t* scale_denoms,
                                          jds_jpeg_scaled_item* scaled);

/* Lossless transcode (DESIGN.md "Transcode"; byte-for-byte definition:
 * tests/transcode_ref.py): the coefficients of jds_decode_jpeg written back as
 * the file form everybody else writes -- ONE interleaved scan (Ns = 3,
 * components 1, 2, 3; Y with Huffman tables 0/0, Cb and Cr with 1/1, whatever
 * the input assigned; no DRI; a grayscale file: SOI | prefix | DHT 0x00 | DHT
 * 0x10 | SOS of Ns = 1 naming the frame's component id | scan | EOI, what
 * libjpeg writes, with optimised tables from the luma counts alone; without a
 * prefix jds_encode_jpeg writes APP0, one DQT and SOF0 with Nf = 1, id 1,
 * sampling 0x11) -- by the interleaved instantiation of the
 * one-pass coder (csrc/jds_entropy_mcu.hip).  No pixel and no coefficient
 * changes.  The output is
 *     SOI | prefix | DHT 0x00, 0x10, 0x01, 0x11 | SOS | scan | EOI
 *   prefix: every marker segment of the input before its first SOS, verbatim
 *     and in order, except DHT and DRI (APPn, COM, DQT, SOF0 untouched); what
 *     follows the first SOS other than scan data is dropped;
 *   tables: optimize == 0 the T.81 Annex K tables; otherwise the K.2 / K.3
 *     tables of jds_encode_jfif_opt built on the device from the symbol counts
 *     of THIS scan (luma from the Y blocks, chroma from Cb and Cr together,
 *     padding blocks included; the > 32-bit fallback per table as there);
 *   padding: the blocks that pad the image to whole MCUs are libjpeg's dummy
 *     blocks: AC zero, DC = the DC of the preceding block of the component in
 *     scan order, so each codes as a zero DC difference and EOB and the next
 *     real block predicts from the last real one;
 *   a restart file is written without intervals, its DC differences taken
 *     across the former boundaries.
 * A block baseline Huffman coding cannot express (DC difference category above
 * 11 -- joining a hostile restart file's intervals can make one -- or AC
 * category above 10) is an error of that file: JDS_EINVAL "not
 * baseline-codable", nothing written.
 *
 * jds_encode_jpeg: one file from host coefficients in jds_decode_jpeg's layout.
 *   Reads H, W, subsampling, grid_cols / grid_rows (they must be T.81's grids of
 *   H x W: JDS_EINVAL otherwise; with reference_grid set a plan's coefficients
 *   are that layout as they are) and, without a prefix, tq and qtable of info.
 *   coeffs: 64 * the grids' blocks entries.  prefix: prefix_len header bytes
 *   to place after SOI (DQT and SOF0 among them: the caller answers for their
 *   agreement with info), or NULL: APP0 (JFIF 1.01), one DQT per table id in
 *   use, SOF0.  *out_len = the file's bytes, also when out_cap is too small
 *   (JDS_EINVAL, nothing written).  Synchronous.
 * jds_jpeg_transcode: parse, decode and write on the context's stream; the
 *   coefficients never leave the device.  The error contract of
 *   jds_decode_jpeg; nothing is written on a defective scan.  info: as
 *   jds_decode_jpeg fills it.  out_cap too small: as above.
 * jds_jpeg_batch_transcode: the batch decode's launches (jds_jpeg_batch_to_rgb
 *   without the inverse), then one set of writer launches over all files.
 *   Items by that call's contract: a file the parser rejects is an item error
 *   (rc), a defective scan sets status, a file that is not baseline-codable
 *   gets rc JDS_EINVAL; the call goes on and returns JDS_OK, jds_last_error
 *   naming the first such file.  Such a file gets out_len 0 and out_off -1 and
 *   no other file's bytes depend on it.  The files are packed in batch order,
 *   each at a multiple of 256; the bytes between a file's end and the next
 *   multiple of 256 are never written; *out_bytes = the last file's end rounded
 *   up to 256.  Synchronous: the per-file lengths are read back once between
 *   the placement and the emit, so no worst-case buffer is needed; out_cap <
 *   *out_bytes: JDS_EINVAL with the need in *out_bytes, items filled, nothing
 *   written.  out: host memory, or with out_on_device != 0 memory of the
 *   context's device.  n == 0 is valid.
 * jds_selftest_jpeg_transcode: test-only, host only: the host decode model
 *   (jds_selftest_jpegdec), then the writer on the host through the kernels'
 *   shared lookup, predecessor rule, splicer and table builder
 *   (csrc/jds_entropy_mcu.hpp, csrc/jds_huffopt.hpp), a serial bit writer
 *   standing in for the lanes.  jds_selftest_jpeg_encode: jds_encode_jpeg's
 *   model likewise.  No GPU. */
typedef struct {
  int32_t rc;        /* JDS_OK, or the code this file alone would get */
  uint32_t status;   /* JDS_DEC_* bits of its scan data; 0: decoded */
  int64_t H, W;
  int32_t subsampling, interleaved;
  int64_t out_off;   /* its first byte in the output, a multiple of 256; -1: not written */
  int64_t out_len;   /* its bytes; 0: not written */
} jds_jpeg_transcode_item;
int jds_encode_jpeg(jds_ctx* ctx, const jds_jpeg_info* info, const int16_t* coeffs, int32_t optimize,
                    const uint8_t* prefix, int64_t prefix_len, uint8_t* out, int64_t out_cap, int64_t* out_len);
int jds_jpeg_transcode(jds_ctx* ctx, const uint8_t* data, int64_t len, int32_t optimize, uint8_t* out, int64_t out_cap,
                       int64_t* out_len, jds_jpeg_info* info);
int jds_jpeg_batch_transcode(jds_ctx* ctx, const uint8_t* const* data, const int64_t* lens, int32_t n,
                             int32_t optimize, uint8_t* out, int64_t out_cap, int32_t out_on_device,
                             jds_jpeg_transcode_item* items, int64_t* out_bytes);
int jds_selftest_jpeg_transcode(const uint8_t* data, int64_t len, int32_t optimize, uint8_t* out, int64_t out_cap,
                                int64_t* out_len);
int jds_selftest_jpeg_encode(const jds_jpeg_info* info, const int16_t* coeffs, int32_t optimize, const uint8_t* prefix,
                             int64_t prefix_len, uint8_t* out, int64_t out_cap, int64_t* out_len);
/* Test-only: the writer's symbol histogram on the device (k_mcu_hist) for host
 * coefficients in jds_decode_jpeg's layout: counts[2][272] = luma, chroma x
 * (16 DC categories, 256 AC symbols). */
int jds_selftest_jpeg_hist_dev(jds_ctx* ctx, const jds_jpeg_info* info, const int16_t* coeffs, uint32_t* counts);

/* Lossless transforms (DESIGN.md "Lossless transforms"; byte-for-byte
 * definition: tests/transform_ref.py): the transcode above with the decoded
 * coefficient planes rewritten into a mirrored, transposed or rotated
 * geometry between the decode and the writer (k_coef_xform,
 * csrc/jds_xform.hip) -- what `jpegtran -flip / -transpose / -rotate` does.
 * No coefficient changes except in sign, so the ideal IDCT of the output is
 * exactly the transformed image.  Per component, with block grid B[r][c]
 * (R x C) and row-major coefficients k[v][u] (v vertical frequency):
 *   hflip      B'[r][C-1-c] = B[r][c],  k'[v][u] = (-1)^u k[v][u]
 *   vflip      B'[R-1-r][c] = B[r][c],  k'[v][u] = (-1)^v k[v][u]
 *   transpose  B'[c][r]     = B[r][c],  k'[u][v] = k[v][u]
 *   rot90 = transpose, then hflip (clockwise, `jpegtran -rotate 90`);
 *   rot270 = hflip, then transpose; rot180 = hflip and vflip;
 *   transverse = transpose, then rot180.
 * Geometry: a mirrored source axis must be whole MCUs (hflip, rot180,
 *   transverse, rot270: W % (8 hs) == 0; vflip, rot180, transverse, rot90:
 *   H % (8 vs) == 0).  Otherwise JDS_ENOTSUP naming the axis (`jpegtran
 *   -perfect`), or with JDS_XF_TRIM or-ed into the operation the source is
 *   first cropped on that axis to whole MCUs (`jpegtran -trim`; JDS_EINVAL when
 *   nothing is left).  Transposition alone has no size constraint.  4:2:2
 *   takes only hflip, vflip and rot180 (a transposed file would be 4:4:0):
 *   JDS_ENOTSUP.  A grayscale file's MCU is 8 x 8 whatever its sampling byte
 *   says (jpegtran's rule for one-component files) and it takes every
 *   operation.  JDS_XF_NONE gives the bytes of jds_jpeg_transcode.
 * Header: the prefix of the transcode with, for transposing operations, every
 *   8-bit table of every DQT segment transposed and SOF0's Y and X swapped;
 *   SOF0 gets the cropped size under trim.  Everything else verbatim.
 * JDS_XF_AUTO: the operation the EXIF Orientation tag asks for (IFD0 tag
 *   0x0112 of the first APP1 "Exif" segment; 1 none, 2 hflip, 3 rot180,
 *   4 vflip, 5 transpose, 6 rot90, 7 transverse, 8 rot270), and the tag is set
 *   to 1 in the output.  No or malformed EXIF, no tag or a value outside 1..8:
 *   the plain transcode, not an error.  No other EXIF field is touched (pixel
 *   dimension tags, the thumbnail).  Explicit operations never touch EXIF.
 *
 * jds_jpeg_transform_info: host only: parse, resolve JDS_XF_AUTO and trim;
 *   *op_out = the operation 0..7, *H_out x *W_out = the output's size; the
 *   geometry errors above.
 * jds_jpeg_transform / jds_jpeg_batch_transform: jds_jpeg_transcode /
 *   jds_jpeg_batch_transcode in every respect (items, packing at multiples of
 *   256, one read of the lengths, the out_cap contract), with an operation per
 *   file (ops == NULL: JDS_XF_AUTO for all).  An item's H and W are the
 *   OUTPUT's size; a file whose operation is refused is an item error with the
 *   code it would get alone.  info (single call): the input's, as
 *   jds_jpeg_transcode fills it.
 * jds_selftest_jpeg_transform: test-only, host only: the host decode model,
 *   the host coefficient transform and prefix editor (csrc/jds_xform.hpp), the
 *   writer's host model.
 * jds_selftest_coef_transform_dev: test-only: k_coef_xform alone on host
 *   coefficients in jds_decode_jpeg's layout of `info` (H, W, subsampling,
 *   grids); op: an explicit operation, JDS_XF_TRIM allowed; coeffs_out: the
 *   destination layout (jds_jpeg_transform_info's size, its T.81 grids). */
#define JDS_XF_NONE 0
#define JDS_XF_HFLIP 1
#define JDS_XF_VFLIP 2
#define JDS_XF_TRANSPOSE 3
#define JDS_XF_TRANSVERSE 4
#define JDS_XF_ROT90 5
#define JDS_XF_ROT180 6
#define JDS_XF_ROT270 7
#define JDS_XF_AUTO 8
#define JDS_XF_TRIM 0x100
int jds_jpeg_transform_info(const uint8_t* data, int64_t len, int32_t op, int32_t* op_out, int64_t* H_out,
                            int64_t* W_out);
int jds_jpeg_transform(jds_ctx* ctx, const uint8_t* data, int64_t len, int32_t op, int32_t optimize, uint8_t* out,
                       int64_t out_cap, int64_t* out_len, jds_jpeg_info* info);
int jds_jpeg_batch_transform(jds_ctx* ctx, const uint8_t* const* data, const int64_t* lens, int32_t n,
                             const int32_t* ops, int32_t optimize, uint8_t* out, int64_t out_cap,
                             int32_t out_on_device, jds_jpeg_transcode_item* items, int64_t* out_bytes);
int jds_selftest_jpeg_transform(const uint8_t* data, int64_t len, int32_t op, int32_t optimize, uint8_t* out,
                                int64_t out_cap, int64_t* out_len);
int jds_selftest_coef_transform_dev(jds_ctx* ctx, const jds_jpeg_info* info, int32_t op, const int16_t* coeffs,
                                    int16_t* coeffs_out);

/* The libjpeg encoding (DESIGN.md "libjpeg encoding"; definition:
 * tests/libjpeg_fwd_ref.py): pixels -> the file libjpeg (libjpeg-turbo, hence
 * Pillow's Image.save(quality=Q, subsampling=S, optimize=O)) writes with its
 * default settings, byte for byte -- jccolor's 16-bit fixed-point RGB ->
 * YCbCr, jcsample's h2v1 / h2v2 box downsampling (bias 0, 1, 0, 1, .. / 1, 2,
 * 1, 2, .. by chroma column), level shift, the ISLOW forward DCT (jfdctint),
 * division by 8 q rounded half away from zero, jpeg_set_quality's tables
 * (luma id 0; Cb and Cr share id 1), then the transcode's writer above with its
 * default prefix.  One kernel (k_jpeg_fwd / k_jpeg_fwd_batch,
 * csrc/jds_jpeg_fwd.hip) writes the coefficients in jds_decode_jpeg's layout
 * and the writer reads them there: they never leave the device.
 *
 * Edges: only the blocks of the T.81 grids are computed (the writer pads to
 *   whole MCUs with its dummy blocks, as jccoefct does).  A sample beyond the
 *   image is the image's edge pixel, with one exception: libjpeg pads the image
 *   to an even number of rows only, downsamples, and then replicates the last
 *   DOWNSAMPLED row, so the rows of a 4:2:0 chroma plane below row
 *   ceil(H / 2) - 1 repeat that row.
 * Scope: ISLOW, no smoothing, 8 bits, one interleaved scan without restart
 *   intervals, JFIF 1.01 header with density 1 x 1; 4:4:4, 4:2:2, 4:2:0 and
 *   grayscale (an H x W one-channel image; SOF0 with Nf = 1, id 1, 0x11).
 * Image bytes: packed, rows H * W * 3 (gray: H * W) with no padding; the
 *   pointer needs no alignment.  A device image is read by aligned words that
 *   each hold at least one byte of the image, and nothing else outside it.
 *
 * jds_jpeg_quality_info: host only.  Fills H, W, subsampling, the sampling
 *   factors, grids, MCU fields, tq = (0, 1, 1), qtable and coeffs_needed of an
 *   image encoded at `quality`; scans and Huffman tables stay zero.  quality
 *   outside 1..100, H or W outside 1..65535 (or H * W above 2^28), or an unknown
 *   subsampling: JDS_EINVAL naming the argument.
 * jds_jpeg_forward_dev: one asynchronous launch on `stream`; nothing is uploaded
 *   or read back.  jds_jpeg_render_dev's checks of tables (integers in
 *   [1, 255], any: not only jds_jpeg_quality_info's) and grids.  rgb_dev: the
 *   image; coeffs_dev: coeffs_needed int16, 16-byte aligned (JDS_EINVAL
 *   otherwise); nothing else is written.
 * jds_rgb_to_jpeg: one image from host memory or (rgb_on_device != 0) memory of
 *   the context's device -> the file in host memory.  *out_len and the
 *   too-small-buffer contract are jds_encode_jpeg's.  Synchronous.
 * jds_rgb_batch_to_jpeg: image i is bytes [rgb_off, rgb_off + H * W * 3 (gray:
 *   H * W)) of rgb_base (any offset: what jds_jpeg_batch_to_rgb reports as
 *   rgb_off serves) with its own size, quality and subsampling.  The forward
 *   launches, one per mode present, then one set of writer launches over all
 *   images.  items_out, the packing at multiples of 256, out_cap / *out_bytes and
 *   out_on_device: jds_jpeg_batch_transcode's contract (status is always 0,
 *   interleaved 1 except for grayscale).  An item with a bad argument
 *   (jds_jpeg_quality_info's checks, a negative rgb_off) gets rc JDS_EINVAL,
 *   takes no space and no other file depends on it; jds_last_error names the
 *   first.  n == 0 is valid.
 * jds_selftest_jpeg_forward: test-only, host only: the tile core
 *   (csrc/jds_jpeg_fwd.hpp) in a host tile loop; coeffs_out: coeffs_needed
 *   int16, 16-byte aligned.  jds_selftest_jpeg_fwd_quant: the core's
 *   division-free quantiser at table entry q for c = 0 .. n - 1 (out[c]) and
 *   -c (out[n + c]); *bound = the |c| its identity is proved for. */
typedef struct {
  int64_t rgb_off;   /* the image's first byte from rgb_base */
  int64_t H, W;
  int32_t quality;   /* 1..100 */
  int32_t subsampling; /* JDS_SS_*; JDS_SS_GRAY: one byte per pixel */
} jds_rgb_item;
int jds_jpeg_quality_info(int32_t quality, int32_t subsampling, int64_t H, int64_t W, jds_jpeg_info* out);
int jds_jpeg_forward_dev(jds_ctx* ctx, const jds_jpeg_info* info, const uint8_t* rgb_dev, int16_t* coeffs_dev,
                         void* stream);
int jds_rgb_to_jpeg(jds_ctx* ctx, const uint8_t* rgb, int32_t rgb_on_device, int64_t H, int64_t W, int32_t quality,
                    int32_t subsampling, int32_t optimize, uint8_t* out, int64_t out_cap, int64_t* out_len);
int jds_rgb_batch_to_jpeg(jds_ctx* ctx, const uint8_t* rgb_base, int32_t rgb_on_device, const jds_rgb_item* items_in,
                          int32_t n, int32_t optimize, uint8_t* out, int64_t out_cap, int32_t out_on_device,
                          jds_jpeg_transcode_item* items_out, int64_t* out_bytes);
int jds_selftest_jpeg_forward(const jds_jpeg_info* info, const uint8_t* rgb, int16_t* coeffs_out);
int jds_selftest_jpeg_fwd_quant(int32_t q, int32_t n, int32_t* out, int32_t* bound);

/* Pillow resizing (DESIGN.md "Pillow resizing"; definition:
 * tests/pillow_resize_ref.py): packed 8-bit RGB -> the bytes Pillow's
 * Image.resize(size, resample, box) gives, byte for byte: ImagingResample's
 * coefficients built in double on the host with the C library's sin / cos,
 * 22-bit fixed-point taps, the horizontal pass rounded to uint8, then the
 * vertical one, a pass Pillow skips skipped, and Image.resize's rule that an
 * image more than 100 times as tall as wide that shrinks is resized vertically
 * first (two launches through a scratch image).  One kernel (k_resize /
 * k_resize_batch, csrc/jds_resize.hip) does both passes of an output tile; the
 * intermediate image is never written.  Image.thumbnail and reducing_gap go
 * through Pillow's separate ImagingReduce and are not provided; neither is
 * NEAREST, nor float or planar output.
 *
 * resample: JDS_RESAMPLE_* (Pillow's numbers); anything else, 0 (NEAREST)
 *   included, is JDS_EINVAL naming the value.
 * box: x0, y0, x1, y1 in pixels of the source, as C floats (Pillow's own
 *   type); NULL: the whole image.  0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H, or
 *   JDS_EINVAL.  out_h, out_w >= 1.
 * JDS_ENOTSUP: an axis that needs more than the tap cap of taps per output
 *   sample (2 * ceil(support * max(scale, 1)) + 1; the message names the need
 *   and the cap), a table with which a 32-bit accumulator could overflow (255 *
 *   sum|k| + 2^21 above 2^31 - 1), an image of more than 2^31 - 1 bytes or tiles.
 * Images are rows of 3 * W bytes without padding at any byte alignment; an
 *   output is out_h * out_w * 3 bytes.  Nothing outside an output is written,
 *   and of a source only the rows and columns the tables name are read.
 *
 * jds_resize_info: host only; the default output tile and the tap cap.
 * jds_rgb_resize: one image from host memory or (rgb_on_device != 0) memory of
 *   the context's device, to host or device memory.  Synchronous.
 * jds_rgb_batch_resize: image i is bytes [rgb_off, rgb_off + H * W * 3) of
 *   rgb_base_dev (any offset: what jds_jpeg_batch_to_rgb reports serves);
 *   output i is bytes [i, i + 1) * out_h * out_w * 3 of out_dev.  The tables
 *   and records are uploaded, then one launch on `stream` (NULL: the null stream)
 *   after the scratch launch of the tall images; the call returns when they
 *   have run (the tables are the context's, and the next call rewrites
 *   them).  n == 0 is valid.
 * jds_jpeg_batch_to_tensor: jds_jpeg_batch_to_rgb_scaled with
 *   JDS_RENDER_LIBJPEG into scratch of the context, then the batch resize on
 *   the same stream: out is n slots of out_h * out_w * 3 bytes in file order
 *   (out_cap at least that, JDS_EINVAL otherwise).  scale_denoms NULL: per file
 *   the largest of 8, 4, 2, 1 that is at most min(W / out_w, H / out_h)
 *   (Pillow's Image.draft).  boxes (nullable): n x 4 floats in the coordinates
 *   of the image as decoded at its denominator.  A file that fails (items[i].rc
 *   or .status, as jds_jpeg_batch_to_rgb reports them) keeps its slot, filled
 *   with zeros; the call returns JDS_OK and jds_last_error names the first.
 *   scaled (nullable): the denominators used and the decoded sizes.
 *   Synchronous.
 * jds_selftest_resize: test-only, host only: the tile core (csrc/jds_resize.hpp)
 *   in a host tile loop with the tiles the device would use.  *worst
 *   (nullable): the largest 255 * sum|k| + 2^21 of the tables built.
 * jds_selftest_resize_coeffs: test-only, host only: one axis' table.  bounds:
 *   2 * out_size int32 (first input sample, count), taps: out_size * *ksize
 *   int32, cap: the entries `taps` holds (JDS_EINVAL, with *ksize set, if too
 *   few).  The tap cap does not apply. */
#define JDS_RESAMPLE_LANCZOS 1
#define JDS_RESAMPLE_BILINEAR 2
#define JDS_RESAMPLE_BICUBIC 3
#define JDS_RESAMPLE_BOX 4
#define JDS_RESAMPLE_HAMMING 5
typedef struct {
  int64_t rgb_off; /* the image's first byte from rgb_base_dev */
  int64_t H, W;
  int32_t has_box; /* 0: the whole image */
  float box[4];    /* x0, y0, x1, y1 */
  int32_t reserved;
} jds_resize_item;
int jds_resize_info(int32_t* tile_h, int32_t* tile_w, int32_t* max_taps);
int jds_rgb_resize(jds_ctx* ctx, const uint8_t* rgb, int32_t rgb_on_device, int64_t H, int64_t W, const float* box,
                   int64_t out_h, int64_t out_w, int32_t resample, uint8_t* out, int32_t out_on_device);
int jds_rgb_batch_resize(jds_ctx* ctx, const uint8_t* rgb_base_dev, const jds_resize_item* items, int32_t n,
                         int64_t out_h, int64_t out_w, int32_t resample, uint8_t* out_dev, void* stream);
int jds_jpeg_batch_to_tensor(jds_ctx* ctx, const uint8_t* const* data, const int64_t* lens, int32_t n, int64_t out_h,
                             int64_t out_w, int32_t resample, const int32_t* scale_denoms, const float* boxes,
                             uint8_t* out, int64_t out_cap, int32_t out_on_device, jds_jpeg_batch_item* items,
                             jds_jpeg_scaled_item* scaled, uint32_t* rounds_out);
int jds_selftest_resize(const uint8_t* rgb, int64_t H, int64_t W, const float* box, int64_t out_h, int64_t out_w,
                        int32_t resample, uint8_t* out, int64_t* worst);
int jds_selftest_resize_coeffs(int32_t in_size, float in0, float in1, int32_t out_size, int32_t resample,
                               int32_t* ksize, int32_t* bounds, int32_t* taps, int64_t cap);

/* Progressive files (DESIGN.md "Progressive files"): entry points of their own
 * beside the baseline ones -- jds_jpeg_parse and every jds_jpeg_* call keep
 * rejecting SOF2 by name.  A progressive file is read as its frame (a
 * jds_jpeg_info filled as jds_jpeg_parse fills it for the baseline file of the
 * same frame: interleaved = 1, n_scans = 1; one component: JDS_SS_GRAY,
 * interleaved = 0; scan[] and huff[] stay zero) plus its scan script, and
 * decodes into the planar coefficient layout of jds_decode_jpeg, so the
 * renderings, the reduced-size decode and the baseline writer take it
 * unchanged.
 *
 * jds_pjpeg_parse (host only; never reads outside [data, data + len)) accepts
 *   SOF2, 8-bit, one or three components with the sampling jds_jpeg_parse
 *   accepts; DC scans (Ss = Se = 0) of one or of all three components; AC scans
 *   with Ns = 1 and 1 <= Ss <= Se <= 63; Al <= 13, Ah = 0 or Al = Ah - 1;
 *   Huffman ids 0..3, redefined between scans at will: a scan records the FILE
 *   OFFSETS (of the Tc/Th byte) of the DHT definitions in effect at its SOS,
 *   -1 for a table it does not read.  The progression must be consistent: a
 *   coefficient's first scan has Ah = 0, a refinement has Ah equal to the Al
 *   last coded for every coefficient of its band, no AC scan comes before the
 *   component's first DC scan -- otherwise JDS_EINVAL naming the scan.  A 65th
 *   scan is JDS_ENOTSUP.  A baseline file is JDS_ENOTSUP "not progressive
 *   (SOF0): use the jpeg_* calls"; the other refusals of jds_jpeg_parse stay.
 *   complete: every coefficient of every component was coded down to Al = 0.
 * The decode (k_pjpeg_chains) walks CHAINS: the DC scans of a file form one,
 *   the AC scans of each component one more; a chain is walked by one lane,
 *   scan after scan, by T.81 Annex G.  A defect -- a code not in the table, a
 *   run or a correction past Se, an EOBRUN longer than the blocks left, data
 *   ending early, a wrong or missing RSTm -- sets JDS_DEC_* bits and ends the
 *   chain; coefficients of such a file are unspecified, nothing outside its
 *   coefficient range is written.
 * jds_pjpeg_decode: one file, host bytes to host coefficients; synchronous;
 *   fills info (info->status: the JDS_DEC_* bits) and returns JDS_EINVAL naming
 *   the defect when status != 0.
 * jds_pjpeg_batch_layout / jds_pjpeg_batch_to_rgb: jds_jpeg_batch_layout_scaled's
 *   and jds_jpeg_batch_to_rgb_scaled's layout, item and error contracts
 *   (scale_denoms NULL: all 1); the chains launch, then the existing batch
 *   render kernels.  A file with complete == 0 is an item error JDS_ENOTSUP
 *   "incomplete progression" (libjpeg smooths such files; the rendering would
 *   not be libjpeg's).
 * jds_pjpeg_batch_transcode: jds_jpeg_batch_transcode's contract; the prefix
 *   is the file's own segments before its first SOS except DHT and DRI, with
 *   its SOF2 marker rewritten as SOF0.  Incomplete files transcode.
 * jds_pjpeg_to_rgb, jds_pjpeg_transcode: the batch of one; the item's rc (or
 *   JDS_EINVAL for defective scan data) is the call's.
 * jds_selftest_pjpegdec: test-only, host only: the same core, chain after chain. */
#define JDS_PJPEG_MAX_SCANS 64
typedef struct {
  int32_t n_components;        /* Ns: 1 or 3 */
  int32_t component[3];        /* 1 Y, 2 Cb, 3 Cr, in scan order */
  int32_t dc_table[3], ac_table[3]; /* Huffman table ids (0..3) per scan component */
  int32_t ss, se, ah, al;
  int32_t restart_interval;    /* DRI in effect at SOS, in MCUs of this scan (Ns = 1: blocks); 0: none */
  int32_t reserved;
  int64_t offset, length;      /* the entropy-coded segment, RSTm markers included */
  int64_t dc_dht[3], ac_dht[3]; /* per scan component: file offset of the table definition it reads; -1: none */
} jds_pjpeg_scan;

typedef struct {
  jds_jpeg_info frame;
  int32_t n_scans;
  int32_t complete;
  uint32_t status;             /* jds_pjpeg_decode: the file's JDS_DEC_* bits */
  uint32_t reserved;
  jds_pjpeg_scan scan[JDS_PJPEG_MAX_SCANS]; /* in file order */
} jds_pjpeg_info;

int jds_pjpeg_parse(const uint8_t* data, int64_t len, jds_pjpeg_info* out);
int jds_pjpeg_decode(jds_ctx* ctx, const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap,
                     jds_pjpeg_info* info);
/* jds_pjpeg_decode with the coefficients left in the caller's buffer on the context's device
 * (coeffs_cap >= coeffs_needed entries; only entries [0, coeffs_needed) are written): what
 * jds_jpeg_render_dev and jds_jpeg_render_scaled_dev take with info->frame.  Synchronous. */
int jds_pjpeg_decode_dev(jds_ctx* ctx, const uint8_t* data, int64_t len, int16_t* coeffs_dev, int64_t coeffs_cap,
                         jds_pjpeg_info* info);
int jds_selftest_pjpegdec(const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap, jds_pjpeg_info* info);
/* On a profiled context (jds_ctx_profile): the walk time in microseconds of every scan of the
 * last progressive call on it, by the device's wall clock inside k_pjpeg_chains.  Order: the
 * files that took part, in batch order; per file its DC chain, then the AC chain of each
 * component; per chain its scans in file order.  *count entries (cap too small: JDS_EINVAL with
 * the need in *count); none when the context was not profiled. */
int jds_pjpeg_scan_times(jds_ctx* ctx, double* us, int64_t cap, int64_t* count);
int jds_pjpeg_batch_layout(const uint8_t* const* data, const int64_t* lens, int32_t n, jds_jpeg_batch_item* items,
                           int64_t* rgb_bytes, int64_t* coef_entries, const int32_t* scale_denoms,
                           jds_jpeg_scaled_item* scaled);
int jds_pjpeg_batch_to_rgb(jds_ctx* ctx, const uint8_t* const* data, const int64_t* lens, int32_t n, uint8_t* rgb,
                           int64_t rgb_cap, int32_t rgb_on_device, int32_t render, const int32_t* scale_denoms,
                           jds_jpeg_batch_item* items, jds_jpeg_scaled_item* scaled, int16_t* coeffs);
int jds_pjpeg_to_rgb(jds_ctx* ctx, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                     int32_t rgb_on_device, int32_t render, int32_t scale_denom, int16_t* coeffs,
                     jds_pjpeg_info* info);
int jds_pjpeg_batch_transcode(jds_ctx* ctx, const uint8_t* const* data, const int64_t* lens, int32_t n,
                              int32_t optimize, uint8_t* out, int64_t out_cap, int32_t out_on_device,
                              jds_jpeg_transcode_item* items, int64_t* out_bytes);
int jds_pjpeg_transcode(jds_ctx* ctx, const uint8_t* data, int64_t len, int32_t optimize, uint8_t* out,
                        int64_t out_cap, int64_t* out_len, jds_pjpeg_info* info);

/* Test-only: the whole decode on the host with the kernels' shared core
 * (csrc/jds_huffdec.hpp; the host model: csrc/jds_jpeg_parse.hpp) and subsequences of subseq_bits bits (a multiple of 8,
 * >= 64), a host loop standing in for the lanes under the same propagation
 * rule.  coeffs: coeffs_cap int16 entries; rounds_out[3]: decode rounds of the
 * Y, Cb, Cr scans (0 for a scan with restart intervals).  No GPU. */
int jds_selftest_huffdec(const uint8_t* data, int64_t len, int32_t subseq_bits, int16_t* coeffs, int64_t coeffs_cap,
                         int32_t* rounds_out);

/* Test-only: evaluate the device DCT expressions (jds_dct8.hpp) on the host so
 * the CPU test suite can pin them against SciPy without a GPU.  Not used by
 * any product path.  in/out: n blocks of 8x8 f64; inverse: 0 = dctn, 1 = idctn. */
int jds_selftest_dct8x8(const double* in, double* out, int64_t n, int32_t inverse);
/* The same for 16x16 blocks (jds_dct16.hpp). */
int jds_selftest_dct16x16(const double* in, double* out, int64_t n, int32_t inverse);

/* Test-only: the certified forward's fp32 chain (jds_fast.hip: colour, prefilter,
 * area average, fdct8_f32 along both axes) evaluated on the host for every 8x8
 * block of one plane (0 Y, 1 Cb, 2 Cr) of an H x W RGB image whose plane size is
 * a multiple of 8.  rows_first bit 0: pass order (1 = k_fwd32i's rows first,
 * 0 = k_fwd32's columns first); bit 1: prefiltered chroma through the combined
 * Gaussian + area taps (what every certified forward kernel computes; 0 = the
 * per-pixel Gaussian then area chains, an fp32 restatement kept for comparison);
 * coefficients before quantisation (n_blocks x 64 f32, raster block order);
 * bound[64] = the rigorous bound on |c_fp32 - c_exact| the kernels certify
 * with (fast_fwd_bounds).  Lets the CPU suite test the bound adversarially. */
int jds_selftest_fwd32(int32_t subsampling, int32_t prefilter, const double* gauss, const uint8_t* rgb, int64_t H,
                       int64_t W, int32_t plane, int32_t rows_first, float* coeffs, double* bound);
/* The same for the certified 16x16 forward (jds_fast16.hip: fdct16_f32, plane
 * size a multiple of 16; rows_first bit 0 as above, 0 = k_fwd16f's order; bit 1:
 * the combined taps, as k_fwd16f computes them): n_blocks x 256 f32
 * coefficients and bound[256] (fast_fwd16_bounds). */
int jds_selftest_fwd16(int32_t subsampling, int32_t prefilter, const double* gauss, const uint8_t* rgb, int64_t H,
                       int64_t W, int32_t plane, int32_t rows_first, float* coeffs, double* bound);

/* Test-only: the certified fast inverse's arithmetic (jds_inv_fast.hip,
 * k_inv_fast: folded dequantisation, AAN IDCT on both axes, clip to [-128, 127],
 * vertical then difference-form chroma blends, colour terms on the 2^-32 magic
 * grid) evaluated on the host with the kernel's own helpers, for an H x W image
 * (even H at 4:2:0, even W at 4:2:x) from coefficients in the
 * IntermediateData.all_quantized_coeffs layout and one 8x8 quant table.
 * fuse: bit 0: 0 = every multiply-add rounded twice, 1 = every one fused (the
 * device compiler may pick either per site); bit 1: the offset form full runs
 * take (the a-priori certificate: S grid steps of 2^-32 ride on the luma
 * constant, jds_selftest_inv_cert reports S).  values: H*W*3 f64, the value v'
 * the certificate judges (RGB order; with bit 1 v' + S * 2^-32, uncertain when
 * its fraction is below 2 S * 2^-32); bytes: H*W*3, the kernel's byte for it.
 * Lets the CPU suite test tools/inv_bound.py's bound (K_LIN / K_CONST)
 * adversarially against the oracle's pre-truncation values. */
int jds_selftest_inv_fast(int32_t subsampling, const int16_t* coeffs, const double* qtable, int64_t H, int64_t W,
                          int32_t fuse, double* values, uint8_t* bytes);

/* Test-only, host only: both forms of the certified inverse's test at the
 * a-priori threshold of full runs (|q Q| <= 1152: T = ceil(E * 2^32) + 1 grid
 * steps, S = T + 1) on n given values (|v| < 2^19, RGB values before
 * truncation).  Per value i: bytes[2i], certain[2i] = the two-sided form on
 * v + MAGIC (uncertain when the fraction word lo <= T or lo >= 2^32 - 1 - T);
 * bytes[2i+1], certain[2i+1] = the one-sided form on v + MAGIC + S * 2^-32
 * (uncertain when lo'' < 2 S).  consts[5] = K_LIN, K_CONST, the |q Q| bound,
 * T, S as compiled into the kernels. */
int jds_selftest_inv_cert(const double* values, int64_t n, uint8_t* bytes, uint8_t* certain, double* consts);

/* Test-only: the same for 16x16 blocks (k_inv16_fast's chain: fidct16 lines,
 * coefficients in 16x16 blocks, Q16[u][v] = qtable[u/2][v/2]); pins
 * tools/inv_bound.py --b16's K_LIN16 / K_CONST16 on the CPU. */
int jds_selftest_inv_fast16(int32_t subsampling, const int16_t* coeffs, const double* qtable, int64_t H, int64_t W,
                            int32_t fuse, double* values, uint8_t* bytes);

/* Test-only, host only: the rows of tile row ty of the tiled 8x8 inverse
 * (k_inv_fast, k_inv2) for an H-row frame, from the kernels' own geometry
 * (csrc/jds_inv_common.hpp InvRows; 4:2:0 tiles start 8 luma rows higher where
 * that adds no tile row).  out[8] = the offset (0 or 8), the number of tile
 * rows, the tile's first luma row and its luma rows, its first chroma block
 * row and its chroma block rows, the first sample row of its chroma window and
 * the window's sample rows.  need (nullable): out[5] x 8 flags, whether the
 * tile computes row r of chroma block row out[4] + i into the window. */
int jds_selftest_inv_rows(int32_t subsampling, int64_t H, int32_t ty, int32_t* out, uint8_t* need);

/* Test-only: the host-built cv2 INTER_AREA table of one axis (OpenCV
 * computeResizeAreaTab, used by the odd-size path) for src -> dst samples:
 * per destination index its tap count n[d] (<= 4) and taps si[4d..], a[4d..].
 * Pinned on the CPU against oracle/cpu_ref.py:area_tab. */
int jds_selftest_area_tab(int32_t src, int32_t dst, int32_t* n, int32_t* si, double* a);

#ifdef __cplusplus
}
#endif

#endif /* JDS_H */
