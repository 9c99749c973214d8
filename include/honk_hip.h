/*
 * honk_hip.h -- C ABI of libhonk_hip.so, the MI355X (gfx950) forward path of
 * Honk's keyword-spotting CNNs.
 *
 * The reference (ljj7975/honk) is pure PyTorch; its "FFI" for this path is the
 * nn.Module call made by its callers.  Each entry point below replaces one
 * reference interface:
 *
 *   honk_res_forward  <- SpeechResModel.forward   /root/reference/utils/model.py:104-121
 *   honk_cnn_forward  <- SpeechModel.forward      /root/reference/utils/model.py:186-205
 *   honk_res_pack     <- SerializableModule.load  /root/reference/utils/model.py:79-80
 *                        (state_dict -> kernel layout, done once per weight change)
 *   honk_*_desc       <- the config dicts          /root/reference/utils/model.py:381-414
 *
 * Conventions: every pointer named x/logits/packed/tensors[i]/workspace is a
 * DEVICE pointer (hipMalloc / torch caching allocator); `stream` is a
 * hipStream_t passed as void*.  Work is enqueued on `stream`; no call
 * allocates device memory, and none synchronises except honk_res_forward in
 * HONK_PREC_F16X2 with its admission on (one hipStreamSynchronize per call, to
 * read the flagged-clip count; honk_res_forward_ordered is the same forward
 * without it) and honk_res_numerics (once per pack).  Global state: a thread-local
 * last-error string, a per-device CU-count cache, and the mutex-guarded
 * timing window of honk_timing_enable/read (off unless enabled; a diagnostic,
 * not used by the forward itself).  Status: 0 = ok, <0 = error, see
 * honk_last_error().
 * Arithmetic: fp32 inputs/outputs everywhere; the res and cnn forwards take a
 * precision field (HONK_PREC_F32: IEEE fp32 MFMA; HONK_PREC_BF16X3: fp32 values
 * as bf16 hi + lo pairs, 3 bf16 MFMA products per MAC, fp32 accumulation -- both
 * meet the 1e-4 logit bar; HONK_PREC_BF16: bf16, top-1 parity); every other
 * entry point is IEEE fp32 (MFMA / FMA), the BatchNorm statistics fp64.
 * Memory contract, one sentence per buffer class ("Memory contract";
 * enforced by tests/test_gpu_memory_contract.py on poisoned, guard-banded buffers):
 *  - workspace: its contents on entry are ignored (every region is written by a
 *    launch of the same call before a launch of that call reads it, indices and
 *    counts included), only bytes [0, *_workspace_bytes) are touched, and what it
 *    holds on return is unspecified.
 *  - outputs (logits, out, y, dx, dw, db, mean, invstd, masks, loss, flagged_count):
 *    contents on entry are ignored and every element of the documented shape is
 *    written, nothing before or behind it.
 *  - packed: honk_res_pack ignores its contents on entry and writes every float a
 *    forward or honk_res_numerics reads, within [0, honk_res_packed_floats); the
 *    pad floats between its regions stay as they were and are never read.
 *  - inputs (x, pcm, packed in a forward, tensors[i], weights, labels, saved
 *    activations): never modified.
 *  - in-place buffers (honk_sgd_step_f32's params and momentum_buf, the running
 *    statistics): elements [0, n) are read and written, nothing outside them.
 */
#ifndef HONK_HIP_H
#define HONK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HONK_OK 0
#define HONK_ERR_ARG (-1)        /* bad descriptor / shape / null pointer        */
#define HONK_ERR_UNSUPPORTED (-2) /* configuration outside the kernels' envelope */
#define HONK_ERR_WORKSPACE (-3)  /* workspace too small                          */
#define HONK_ERR_HIP (-4)        /* a HIP runtime call failed                    */

/* ---- SpeechResModel (res8/15/26[-narrow]); utils/model.py:82-121 ------------- */
typedef struct honk_res_desc {
  int32_t n_labels;       /* config["n_labels"]                                  */
  int32_t n_maps;         /* config["n_feature_maps"] (1..64 in f32, 1..48 bf16*) */
  int32_t n_layers;       /* config["n_layers"]                                  */
  int32_t use_dilation;   /* config["use_dilation"]: conv{i} dilation 2**((i-1)//3) */
  int32_t pool_h, pool_w; /* config["res_pool"], or 0,0 when absent              */
  int32_t height, width;  /* input frames x MFCC coefficients (101, 40)          */
  int32_t precision;      /* HONK_PREC_F32 (IEEE fp32 MFMA, 1e-4 parity),
                             HONK_PREC_BF16 (bf16 activations/weights, fp32
                             accumulate; top-1 parity) or HONK_PREC_BF16X3
                             (fp32 values as bf16 hi + lo pairs, products
                             hi*hi + hi*lo + lo*hi on bf16 MFMA, fp32
                             accumulate; 1e-4 parity) -- same packed buffer.
                             BF16 / BF16X3: the row-band staging plan bounds
                             the (pooled) width -- 66 for 45-map bf16x3, 154
                             for 45-map bf16 -- HONK_ERR_UNSUPPORTED beyond */
} honk_res_desc;

#define HONK_PREC_F32 0
#define HONK_PREC_BF16 1
#define HONK_PREC_BF16X3 2
/* fp16 activations (RNE), weights (input BN folded) as fp16 hi + lo, products
   w_hi*x + w_lo*x on fp16 MFMA, fp32 accumulate: ~11-bit activations, each clip's
   stored tensors scaled by a power of two that keeps them inside fp16's range (see
   HONK_NUM_SCALE).  Runs on the weight-stationary / pair kernels only (n_maps <= 48
   with a zero-padding channel, (pooled) width < 64; HONK_ERR_UNSUPPORTED otherwise).
   Logit error: within the 1e-4 bar on res15 (simulated <= 3.8e-5, measured on the
   goldens); up to ~2e-4 on the pooled res8 / res26 maps, which average over fewer
   pixels -- honk_res_select_precision routes those to BF16X3. */
#define HONK_PREC_F16X2 3
/* Not a kernel format: honk_res_select_precision's request for "the fastest mode that
   holds the 1e-4 logit bar for this model" (f16x2 -> bf16x3 -> f32). */
#define HONK_PREC_AUTO 4

/* number of floats of the packed (kernel-layout) weight buffer */
size_t honk_res_packed_floats(const honk_res_desc* d);
/* bytes of scratch needed by honk_res_forward for `batch` clips */
size_t honk_res_workspace_bytes(const honk_res_desc* d, int64_t batch);
/*
 * The block-layer launches honk_res_forward makes per batch chunk, in order: kinds[i]
 * = HONK_KERNEL_* (up to max_kinds written).  Returns the launch count (> 0), or a
 * (negative) HONK_ERR_* status code.  n_cus = 0: the current device's CU count (the pair kernel's plan
 * depends on clips per workgroup).  Host-only; no GPU work.
 */
#define HONK_KERNEL_BLOCK_F32 1 /* fp32-MFMA layer (block_kernel)                        */
#define HONK_KERNEL_ROWBAND 2   /* bf16 / bf16x3 row-band layer (block16r_kernel)          */
#define HONK_KERNEL_WSTAT 3     /* bf16 / bf16x3 weight-stationary layer (block16w_kernel) */
#define HONK_KERNEL_PAIR 4      /* fused odd + even layer pair (block16p_kernel)           */
#define HONK_KERNEL_LAST 5      /* last (odd) layer, fused channel sums (block16l_kernel)  */
/* 6 and 7 are retired (the removed block16n_kernel and block16k_kernel) and stay unassigned */
int honk_res_launch_plan(const honk_res_desc* d, int64_t batch, int32_t n_cus, int32_t* kinds, int32_t max_kinds);
/*
 * Pack a state_dict into kernel layout.  tensors[] (device, fp32, contiguous),
 * in this order (n_tensors = 3*n_layers + 3):
 *   conv0.weight [C,1,3,3], conv1.weight .. conv{L}.weight [C,C,3,3],
 *   bn1.running_mean, bn1.running_var, .., bn{L}.running_mean, bn{L}.running_var [C],
 *   output.weight [n_labels,C], output.bias [n_labels]
 */
int honk_res_pack(const honk_res_desc* d, const float* const* tensors, int32_t n_tensors,
                  float* packed, void* stream);
/*
 * The numerics record honk_res_pack writes into `packed` (device; read by the f16x2
 * forward, and by the host through honk_res_numerics):
 *   HONK_NUM_SCALE    s_model, the power-of-two activation scale of the f16x2 path:
 *                     M * s_model < 2^4 (each clip stores s * (its pre-BN tensors) with
 *                     s = s_model, lowered by the binades its input's conv0 bound
 *                     max|x| * HONK_NUM_W0SUM exceeds M -- fp16's range follows the clip)
 *   HONK_NUM_RANGE    M = max over layers / channels of |running_mean| + 8 sqrt(running_var)
 *   HONK_NUM_W0SUM    max_c sum_t |conv0.weight[c][0][t]|
 *   HONK_NUM_RHO      max over layers of sqrt(mean_c (mean_c^2 + var_c) / var_c): the RMS
 *                     size of a stored tensor in its own BatchNorm units (the factor by
 *                     which the storage rounding grows in the next layer); NaN if a
 *                     statistic is not finite
 *   HONK_NUM_F16_OVERFLOW  1 if a folded weight (W * invstd, or a border-bias weight)
 *                     has no finite fp16 (hi, lo) split
 *   HONK_NUM_RHO_LAYER the layer (1-based) of HONK_NUM_RHO
 *   HONK_NUM_VALID    1 once the record is written
 *   HONK_NUM_OUT_SCALE 2^kw[L] for an odd n_layers (the last layer's output relative to
 *                     the residual stream's scale), else 1
 *   [HONK_NUM_KW + i] kw[i+1], the f16x2 weight exponent of conv{i+1}: its folded weights
 *                     are packed times 2^kw, an odd layer and the even layer after it
 *                     taking +k / -k (keeps weights of layers fed by a wide-spread tensor
 *                     out of fp16's subnormal range; 0 / +-1 at unit scale)
 */
#define HONK_NUM_SCALE 0
#define HONK_NUM_RANGE 1
#define HONK_NUM_W0SUM 2
#define HONK_NUM_RHO 3
#define HONK_NUM_F16_OVERFLOW 4
#define HONK_NUM_RHO_LAYER 5
#define HONK_NUM_VALID 6
#define HONK_NUM_OUT_SCALE 7
#define HONK_NUM_COUNT 8
#define HONK_NUM_KW 64
/* Copy the first n (at most HONK_NUM_KW + n_layers) record entries to HOST memory rec[]:
   enqueues the copy on `stream` and SYNCHRONISES it (once per pack, not on the forward
   path). */
int honk_res_numerics(const honk_res_desc* d, const float* packed, float* rec, int32_t n, void* stream);
/*
 * Host-only precision policy: the precision honk_res_forward should run for the
 * `requested` one (HONK_PREC_*, HONK_PREC_AUTO) given the model's record (rec from
 * honk_res_numerics; may be NULL for F32 / BF16).  F32 -> F32; BF16 (top-1 parity, an
 * explicit choice) -> BF16 where the kernels take the shape, else F32; F16X2 / AUTO ->
 * F16X2 where its 1e-4 contract holds (unpooled maps of >= 4040 pixels and >= 32 maps,
 * no folded weight beyond fp16's range, HONK_NUM_RHO <= 3.5), else as BF16X3; BF16X3
 * -> BF16X3 where supported and HONK_NUM_RHO <= 100, else F32.  note (may be NULL)
 * receives why a requested format was not taken ("" when it was).  Returns the
 * precision (>= 0) or a HONK_ERR_* code.
 */
int honk_res_select_precision(const honk_res_desc* d, const float* rec, int32_t requested, char* note,
                              size_t note_len);
/*
 * x: [batch, height, width] fp32;  logits: [batch, n_labels] fp32 (eval-mode forward)
 *
 * HONK_PREC_F16X2 admits every clip on its own (per batch, not once per model): after the
 * f16x2 pass, a clip whose last-layer BatchNorm'd channel means lie beyond
 * HONK_F16X2_Z_MAX standard deviations of the model's calibration (an input far outside
 * the distribution the running statistics describe: f16x2's rounding is no longer
 * averaged away there), or whose f16x2 logits are not finite while its input is, or whose
 * scale was lowered by more than HONK_F16X2_DROP_MAX binades (below), is re-run in BF16X3
 * and its logits replaced.  This is the one honk_res_forward mode that
 * SYNCHRONISES `stream` (once per call, to read the flagged-clip count; not capturable
 * in a hipGraph -- honk_res_forward_ordered below is).  HONK_F16X2_RERUN=0 in the
 * environment turns the admission off (raw f16x2: kernel tests).  The workspace
 * (honk_res_workspace_bytes) includes its buffers.
 */
int honk_res_forward(const honk_res_desc* d, const float* packed, const float* x, float* logits,
                     int64_t batch, void* workspace, size_t workspace_bytes, void* stream);
#define HONK_F16X2_Z_MAX 8
/* The second admission statistic, the clip's crest against the model: a clip's scale is
   s_model lowered by ex binades, max|x| * HONK_NUM_W0SUM / HONK_NUM_RANGE < 2^ex
   (HONK_NUM_SCALE above).  One loud entry or frame in an otherwise calibrated clip (a click)
   lowers the scale but barely moves a last-layer channel mean, an average over the whole
   map, while the fp16 rounding of the large values around it is absolute in size: measured
   on tests/golden/range_res15-spike.npz, clips at ex <= 4 stay within half the 1e-4 bar,
   clips at ex = 6 reach 1.6 bars with |z| <= 7.  A clip with ex > HONK_F16X2_DROP_MAX is
   flagged by the scale pass itself (no cost on the forward path); calibrated inputs sit at
   ex <= 3 (the round-6 admission). */
#define HONK_F16X2_DROP_MAX 4
/* The clips the calling thread's last honk_res_forward re-ran in bf16x3 (0 unless F16X2;
   0 after honk_res_forward_ordered: the host does not learn the count). */
int64_t honk_res_rerun_count(void);
/*
 * The same forward, STREAM-ORDERED in every mode: it only enqueues kernels on `stream` --
 * no copy to the host, no stream / device / event synchronisation, no allocation, no
 * stream or event creation -- so it returns before the work has run and can be captured
 * in a hipGraph.  (An open honk_timing_enable window records events around the block
 * launches, as in honk_res_forward; leave it closed while capturing.)  Same workspace
 * (honk_res_workspace_bytes), same status codes.
 *
 * F32 / BF16 / BF16X3, and F16X2 with HONK_F16X2_RERUN=0: the launches and the logits of
 * honk_res_forward.  F16X2 with the admission: the f16x2 pass, the flags and the compacted
 * list of flagged clips as in honk_res_forward; then, since the host does not know how
 * many clips were flagged, ceil(cap / rc) re-run rounds are enqueued unconditionally
 * (cap = rerun_capacity, or batch when rerun_capacity <= 0 or > batch; rc =
 * honk_res_rerun_clips).  Every kernel of the round at offset o reads the flagged count
 * from device memory and works on its first clamp(min(count, cap) - o, 0, rc) clips; the
 * workgroups of the others return at once (a round nothing is left for costs its empty
 * launches).  Flagged clips past the first cap, in batch order, KEEP THEIR F16X2 LOGITS.
 *
 * flagged_count (device int32, may be NULL): receives the batch's flagged-clip count, not
 * limited to cap (written by a kernel on `stream`; 0 in the modes without an admission):
 * *flagged_count > cap, read later, tells the caller that the re-run overflowed.
 * batch == 0: HONK_OK; 0 is written to flagged_count when it is not NULL (`stream` must
 * then be valid), nothing else is enqueued.
 */
int honk_res_forward_ordered(const honk_res_desc* d, const float* packed, const float* x, float* logits,
                             int64_t batch, void* workspace, size_t workspace_bytes, void* stream,
                             int64_t rerun_capacity, int32_t* flagged_count /* device, may be NULL */);
/* Host-only: the clips one bf16x3 re-run round of the f16x2 admission takes for `batch`
   clips (both entry points), or 0: not F16X2, the admission off, or an unsupported shape. */
int64_t honk_res_rerun_clips(const honk_res_desc* d, int64_t batch);
/*
 * The LATENCY schedule of the same forward, for batches smaller than the device's CU count.
 * The schedule above is planned for throughput: on the 16-bit paths a workgroup owns whole
 * clips (the fused pairs, the last-layer kernel) or tall row bands, so a batch of B clips
 * keeps B of the CUs busy and its latency does not fall with B.  Here every block layer of a
 * chunk of fewer clips than CUs (and fewer than 1024) in BF16 / BF16X3 / F16X2 is one launch of
 * the split band kernel (HONK_KERNEL_SPLIT): tiles of (clip, dilation class, band of class
 * rows, 16 out channels), at least one per CU where the map has that many.  Per output the
 * arithmetic and its order are those of the kernel the throughput schedule runs (the
 * weight-stationary / pair kernels', or the row-band kernel's), and the last layer's channel
 * sums are added in its order: the logits are BIT FOR BIT honk_res_forward_ordered's.  Chunks
 * of at least as many clips as CUs and F32 run the throughput schedule unchanged (as does a
 * row-band map too wide for the split kernel's staging image).
 *
 * honk_res_forward_latency: honk_res_forward_ordered's contract in every respect (enqueue
 * only, capturable, status codes, batch == 0, rerun_capacity, flagged_count; the re-run
 * rounds run in this schedule too) with the workspace of honk_res_latency_workspace_bytes.
 * honk_res_latency_plan: the block-layer launches of one chunk -- kinds[i] = HONK_KERNEL_*,
 * tiles[i] = the launch's tiles (workgroups' worth of work: band tiles x out-tiles for
 * HONK_KERNEL_SPLIT, bands for the band kernels, workgroups for the pair / last kernels); either
 * may be NULL; up to max_steps written.  Returns the launch count or a (negative) HONK_ERR_*
 * code, refusing what honk_res_launch_plan refuses.  Both queries are host-only.
 */
#define HONK_KERNEL_SPLIT 8     /* one layer, split over all CUs (block16s_kernel)         */
int honk_res_forward_latency(const honk_res_desc* d, const float* packed, const float* x, float* logits,
                             int64_t batch, void* workspace, size_t workspace_bytes, void* stream,
                             int64_t rerun_capacity, int32_t* flagged_count /* device, may be NULL */);
size_t honk_res_latency_workspace_bytes(const honk_res_desc* d, int64_t batch);
int honk_res_latency_plan(const honk_res_desc* d, int64_t batch, int32_t n_cus, int32_t* kinds, int64_t* tiles,
                          int32_t max_steps);

/* ---- SpeechModel (cnn-*); utils/model.py:123-205 ------------------------------ */
typedef struct honk_cnn_desc {
  int32_t height, width, n_labels;
  int32_t c1_out, c1_kh, c1_kw, c1_sh, c1_sw, p1_h, p1_w;   /* conv1 + pool1         */
  int32_t has_conv2, c2_out, c2_kh, c2_kw, c2_sh, c2_sw, p2_h, p2_w;
  int32_t has_lin;                                        /* Linear(flat, 32), no ReLU */
  int32_t dnn1, dnn2;                                     /* 0 = absent              */
  int32_t dnn1_relu;                                      /* 1 unless tf_variant     */
  int32_t precision;  /* HONK_PREC_F32 or HONK_PREC_BF16X3 (convs and >16-output Linears on the
                         bf16 MFMA pipe with hi/lo-split operands; 1e-4 parity)  */
} honk_cnn_desc;

size_t honk_cnn_workspace_bytes(const honk_cnn_desc* d, int64_t batch);
/*
 * The launches honk_cnn_forward makes, in order: kinds[i] = HONK_CNN_KERNEL_* (up to max_kinds
 * written) -- first the per-call weight pack of a dedicated conv2 kernel (if one runs), then
 * what every chunk of clips launches: conv1, [pool1], [conv2, [pool2]], [lin], [dnn1], [dnn2],
 * output.  Returns the launch count (> 0), or a (negative) HONK_ERR_* status code.  The forward
 * runs the very list this reports, under the same HONK_CNN_C1F / C1X3 / C2F / C2X3 switches
 * (= 0: that dedicated kernel off).  Host-only; no GPU work.
 *
 * The generic implicit GEMM of a conv is HONK_CNN_KERNEL_GEMM plus flags: its precision, the
 * fused 2x2 max-pool, and the layout it stores (NCHW fp32, or the NHWC input of the dedicated
 * conv2 kernels).  A Linear with > 16 outputs is the same GEMM, reported as LINEAR_GEMM_*.
 */
#define HONK_CNN_KERNEL_CONV1X3 1        /* conv1x3_kernel (bf16x3 conv1 + ReLU + 2x2 pool)     */
#define HONK_CNN_KERNEL_CONV1F 2         /* conv1f_kernel  (fp32   conv1 + ReLU + 2x2 pool)     */
#define HONK_CNN_KERNEL_CONV2X3 3        /* conv2x3_kernel<13>                                  */
#define HONK_CNN_KERNEL_CONV2F 4         /* conv2f_kernel<13>                                   */
#define HONK_CNN_KERNEL_MAXPOOL 5        /* maxpool_kernel (a pool the conv's GEMM did not fuse) */
#define HONK_CNN_KERNEL_PACK_CONV2X3 6   /* pack_conv2x3_kernel                                 */
#define HONK_CNN_KERNEL_PACK_CONV2F 7    /* pack_conv2f_kernel                                  */
#define HONK_CNN_KERNEL_LINEAR_SMALL4 8  /* linear_small_kernel<4, 4>   (<= 4 outputs)          */
#define HONK_CNN_KERNEL_LINEAR_SMALL8 9  /* linear_small_kernel<8, 4>   (5 .. 8)                */
#define HONK_CNN_KERNEL_LINEAR_SMALL16 10 /* linear_small_kernel<16, 4> (9 .. 16)               */
#define HONK_CNN_KERNEL_LINEAR_GEMM_F32 11 /* conv_gemm_kernel<false, false> as a Linear        */
#define HONK_CNN_KERNEL_LINEAR_GEMM_X3 12  /* conv_gemm_kernel<false, true>  as a Linear        */
#define HONK_CNN_KERNEL_GEMM 16          /* conv_gemm_kernel of a conv, or-ed with:             */
#define HONK_CNN_GEMM_X3 1               /*   bf16x3 operands (else fp32)                       */
#define HONK_CNN_GEMM_POOL2 2            /*   fused 2x2 max-pool                                */
#define HONK_CNN_GEMM_NHWC_BF16 4        /*   stores [B][PH][PW][hi N | lo N] bf16 (conv2x3's input) */
#define HONK_CNN_GEMM_NHWC_F32 8         /*   stores [B][PH][PW][N] fp32 (conv2f's input)       */
int honk_cnn_launch_plan(const honk_cnn_desc* d, int32_t* kinds, int32_t max_kinds);
/*
 * tensors[] (device fp32, contiguous; NULL for absent layers), fixed order of 12:
 *   conv1.weight, conv1.bias, conv2.weight, conv2.bias, lin.weight, lin.bias,
 *   dnn1.weight, dnn1.bias, dnn2.weight, dnn2.bias, output.weight, output.bias
 * No separate pack call: OIHW weights are the [N][K] operand of the generic implicit GEMM; the
 * bf16x3 cnn-trad-pool2 path splits conv2's weights into hi/lo fragments inside the workspace
 * on every call (one small launch) and conv1's while staging them into registers.
 */
int honk_cnn_forward(const honk_cnn_desc* d, const float* const* tensors, const float* x,
                     float* logits, int64_t batch, void* workspace, size_t workspace_bytes,
                     void* stream);
/*
 * The LATENCY schedule of the same forward, for batches smaller than the device's CU count.
 * honk_cnn_forward is planned for throughput: the four hand-scheduled kernels give a workgroup
 * a whole clip, a few-output Linear is one workgroup per 4 clips with the whole K serial in it,
 * and a wider Linear is one GEMM block per 128 clips.  Here a chunk of fewer clips than
 * honk_cnn_latency_threshold runs
 *   - each dedicated conv of the throughput plan as its split form: conv2 in tiles of (clip,
 *     16-pixel m-tile, 16-channel out tile), one wave each, staging only the image rows the tile
 *     reaches; conv1 in tiles of (clip, band of pooled m-tiles, 2 out tiles), at least one per
 *     CU where the chunk yields that many (bands of 4 m-tiles).  Per output element the MFMAs,
 *     their order, the fragments and the epilogue are the throughput kernel's: the conv stack's
 *     output is BIT FOR BIT the same (honk_cnn_features_f32 lets a test compare it);
 *   - each Linear whose K spans at least two slices as split-K: workgroup (slice, 4 rows, 8
 *     outputs) writes an fp32 partial [slice][row][n] into the workspace, a second launch adds
 *     the partials in ascending slice order, then the bias, then the ReLU.  No atomics; the slice
 *     length depends on (K, n) only, so a clip's logits depend neither on the batch around it
 *     nor on the device.  fp32 fmaf accumulation in both precisions: NOT bit-equal to
 *     honk_cnn_forward (the sums are associated differently), within the same 1e-4 bar;
 *   - everything else (the generic GEMM convs, maxpool_kernel, the weight pack, a shorter
 *     Linear) on its throughput kernel.
 * A dedicated kernel switched off (HONK_CNN_C1F / C1X3 / C2F / C2X3 = 0) has no split form
 * either; a conv2 tile whose two half images exceed 64 KiB of LDS stays on the throughput kernel.
 * Chunks of at least honk_cnn_latency_threshold clips run the throughput plan unchanged: there
 * the logits are bit for bit honk_cnn_forward's.
 *
 * honk_cnn_forward_latency: honk_cnn_forward's contract in every respect (the 12 tensors,
 * enqueue only -- no synchronisation, capturable --, status codes and refusals, batch == 0
 * writes nothing) with the workspace of honk_cnn_latency_workspace_bytes (activations,
 * fragments, split-K partials; a workspace one byte short is refused with nothing enqueued).
 * honk_cnn_latency_plan: the launches of one chunk of `batch` clips on a device of n_cus CUs
 * (0: ask the device) -- kinds[i] = HONK_CNN_KERNEL_*, tiles[i] = the launch's workgroups;
 * either may be NULL; up to max_steps written.  Returns the launch count or a (negative)
 * HONK_ERR_* code, refusing what honk_cnn_launch_plan refuses.  The forward runs the very
 * list this reports.  honk_cnn_latency_threshold: min(n_cus, 1 + the largest measured batch at
 * which the split schedule was not slower: 96 clips in F32, 64 in BF16X3; only d->precision is
 * read).  The three queries are host-only (n_cus > 0).
 */
#define HONK_CNN_KERNEL_CONV1XS 13       /* conv1xs_kernel: conv1x3_kernel, split               */
#define HONK_CNN_KERNEL_CONV1FS 14       /* conv1fs_kernel: conv1f_kernel, split                */
#define HONK_CNN_KERNEL_CONV2XS 15       /* conv2xs_kernel: conv2x3_kernel, split               */
#define HONK_CNN_KERNEL_CONV2FS 32       /* conv2fs_kernel: conv2f_kernel, split                */
#define HONK_CNN_KERNEL_LINEAR_SPLITK 33 /* linear_splitk_kernel (the K slices' partials)       */
#define HONK_CNN_KERNEL_LINEAR_SPLITK_SUM 34 /* linear_splitk_sum_kernel (+ bias, ReLU)         */
int honk_cnn_forward_latency(const honk_cnn_desc* d, const float* const* tensors, const float* x,
                             float* logits, int64_t batch, void* workspace, size_t workspace_bytes,
                             void* stream);
size_t honk_cnn_latency_workspace_bytes(const honk_cnn_desc* d, int64_t batch);
int honk_cnn_latency_plan(const honk_cnn_desc* d, int64_t batch, int32_t n_cus, int32_t* kinds,
                          int64_t* tiles, int32_t max_steps);
int64_t honk_cnn_latency_threshold(const honk_cnn_desc* d, int32_t n_cus);
/* Exported for tests: the conv / pool steps of either schedule (latency = 0: honk_cnn_forward's,
   1: honk_cnn_forward_latency's), stopping before the first Linear: features[batch][flat] fp32
   in the flatten order of model.py:194 (NCHW).  Workspace: honk_cnn_latency_workspace_bytes
   (latency = 0 takes honk_cnn_workspace_bytes as well). */
int honk_cnn_features_f32(const honk_cnn_desc* d, const float* const* tensors, const float* x,
                          float* features, int64_t batch, void* workspace, size_t workspace_bytes,
                          void* stream, int32_t latency);

/* ---- layer-level operators (used by the cnn driver; exported for tests) ------- */
/* out[b][n][oh][ow] = act(bias[n] + sum_{ci,kh,kw} in[b][ci][oh*sh+kh][ow*sw+kw] * w[n][ci][kh][kw]) */
int honk_conv2d_f32(const float* in, const float* w, const float* bias, float* out, int64_t batch,
                    int32_t cin, int32_t h, int32_t w_, int32_t cout, int32_t kh, int32_t kw,
                    int32_t sh, int32_t sw, int32_t relu, void* stream);
/* nn.MaxPool2d((kh,kw)) on NCHW, stride = kernel, floor */
int honk_maxpool2d_f32(const float* in, float* out, int64_t batch, int32_t c, int32_t h, int32_t w,
                       int32_t kh, int32_t kw, void* stream);
/* y[m][n] = act(b[n] + sum_k x[m][k] * w[n][k])  (nn.Linear) */
int honk_linear_f32(const float* x, const float* w, const float* b, float* y, int64_t m, int32_t k,
                    int32_t n, int32_t relu, void* stream);
/* The same Linear on the latency schedule's split-K kernels (few rows m): fp32 partials
   [slice][m][n] in the workspace, summed in ascending slice order, then bias, then ReLU.
   honk_linear_splitk_slices: the K slices of a (k, n) Linear -- a function of k and n only -- or
   0 where k is shorter than two slices (the forward keeps such a layer on its throughput kernel;
   this call runs it all the same, in ceil(k / slice) slices).  Workspace:
   honk_linear_splitk_workspace_bytes. */
int32_t honk_linear_splitk_slices(int32_t k, int32_t n);
size_t honk_linear_splitk_workspace_bytes(int64_t m, int32_t k, int32_t n);
int honk_linear_splitk_f32(const float* x, const float* w, const float* b, float* y, int64_t m,
                           int32_t k, int32_t n, int32_t relu, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- SpeechModel training (utils/train.py:123-135 on the cnn configs) ----------- */
/*
 * The backward of model.py:186-193 (relu(conv) -> dropout -> max-pool; the forward is
 * honk_conv2d_f32 with relu = 1 and honk_maxpool2d_f32), replacing the cuDNN/MIOpen
 * convolution backward and max_pool2d_with_indices_backward autograd runs there.
 * g' below is the output gradient gy through the ReLU: g' = (act <= 0 ? 0 : gy), act =
 * the forward's ReLU output (act may be NULL: g' = gy) -- torch's threshold_backward.
 *
 * Max-pool backward (MaxPool2d((kh,kw)), stride = kernel, floor): gin = gout at each
 * window's first maximum in scan order (v > m || isnan(v): torch's index), 0 elsewhere.
 */
int honk_maxpool2d_bwd_f32(const float* in, const float* gout, float* gin, int64_t batch, int32_t c, int32_t h,
                           int32_t w, int32_t kh, int32_t kw, void* stream);
/* dw[n][ci][kh][kw] = sum_{b,oh,ow} g'[b][n][oh][ow] * in[b][ci][oh*sh+kh][ow*sw+kw]; db[n] = sum g' (db may
 * be NULL).  fp32 MFMA; deterministic (per-split partials in the workspace, summed in fixed order). */
size_t honk_conv2d_wgrad_workspace_bytes(int64_t batch, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t kh,
                                         int32_t kw, int32_t sh, int32_t sw);
int honk_conv2d_wgrad_f32(const float* in, const float* gy, const float* act, float* dw, float* db, int64_t batch,
                          int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t kh, int32_t kw, int32_t sh,
                          int32_t sw, void* workspace, size_t workspace_bytes, void* stream);
/* stride 1: dx[b][ci][y][x] = sum_{n,kh,kw} g'[b][n][y-kh][x-kw] * w[n][ci][kh][kw] (zero outside g'),
 * dx [batch][cin][h][w]; the full correlation as an fp32-MFMA implicit GEMM over g' padded in the workspace */
size_t honk_conv2d_dgrad_workspace_bytes(int64_t batch, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t kh,
                                         int32_t kw);
int honk_conv2d_dgrad_f32(const float* gy, const float* act, const float* w, float* dx, int64_t batch, int32_t cin,
                          int32_t h, int32_t w_, int32_t cout, int32_t kh, int32_t kw, void* workspace,
                          size_t workspace_bytes, void* stream);
/*
 * Host-only introspection (no launch, no device): how the two gradients above run one
 * conv shape -- the values the launches themselves read.  Writes the first
 * min(n_out, HONK_CONV2D_TRAIN_PLAN_COUNT) of the values below and returns
 * HONK_CONV2D_TRAIN_PLAN_COUNT, or the HONK_ERR_* code the gradients refuse the shape
 * with (batch < 1 is refused here: nothing is planned for it).  The weight gradient:
 * M = batch*oh*ow reduction rows, a grid of (TN, TK, S) workgroups (64 out channels x 64
 * (ci,kh,kw) columns x one split of MPER rows, a multiple of the 32-row stage; the last
 * split takes what is left).  The input gradient (sh == sw == 1; zeros otherwise): the
 * GEMM's reduction DGRAD_K = cout*kh*kw and rows DGRAD_M = batch*h*w, whether its
 * k->offset table is in LDS (DGRAD_K <= 4096) or computed, whether the flipped weights
 * (behind the padded g' in the workspace) are 16-byte aligned given a 256-byte-aligned
 * workspace (else the GEMM reads them one float at a time), its gridDim.x, and the block
 * count and passes per thread of the padding kernel's grid-stride loop.
 */
enum {
  HONK_CONV2D_TRAIN_PLAN_M = 0,
  HONK_CONV2D_TRAIN_PLAN_TN = 1,
  HONK_CONV2D_TRAIN_PLAN_TK = 2,
  HONK_CONV2D_TRAIN_PLAN_S = 3,
  HONK_CONV2D_TRAIN_PLAN_MPER = 4,
  HONK_CONV2D_TRAIN_PLAN_DGRAD_K = 5,
  HONK_CONV2D_TRAIN_PLAN_DGRAD_KTAB = 6,
  HONK_CONV2D_TRAIN_PLAN_DGRAD_WF_ALIGNED = 7,
  HONK_CONV2D_TRAIN_PLAN_DGRAD_GRID_X = 8,
  HONK_CONV2D_TRAIN_PLAN_DGRAD_PAD_BLOCKS = 9,
  HONK_CONV2D_TRAIN_PLAN_DGRAD_PAD_PASSES = 10,
  HONK_CONV2D_TRAIN_PLAN_DGRAD_M = 11,
  HONK_CONV2D_TRAIN_PLAN_COUNT = 12
};
int honk_conv2d_train_plan(int64_t batch, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t kh, int32_t kw,
                           int32_t sh, int32_t sw, int64_t* out, int32_t n_out);
/* The same for honk_maxpool2d_bwd_f32 (a call of its own, so a query of its own): the block
 * count and the passes per thread of its grid-stride loop over batch*c*h*w elements. */
enum { HONK_MAXPOOL2D_BWD_PLAN_BLOCKS = 0, HONK_MAXPOOL2D_BWD_PLAN_PASSES = 1, HONK_MAXPOOL2D_BWD_PLAN_COUNT = 2 };
int honk_maxpool2d_bwd_plan(int64_t batch, int32_t c, int32_t h, int32_t w, int32_t kh, int32_t kw, int64_t* out,
                            int32_t n_out);

/*
 * The res block conv for ANY channel count C (3x3, padding = dilation = dil, no bias,
 * NCHW fp32; model.py:94-98) -- the general path under honk_conv3x3_f32's
 * {19, 45}-map kernels: the input zero-padded into the workspace, then the fp32-MFMA
 * implicit GEMM with dilation.  flip = 1: the input gradient (w'[i][o][t] =
 * w[o][i][8-t], as honk_conv3x3_f32).  The weight gradient as
 * honk_conv3x3_wgrad_f32 (deterministic).  Workspace: honk_conv_same_workspace_bytes.
 */
size_t honk_conv_same_workspace_bytes(int64_t batch, int32_t c, int32_t h, int32_t w_, int32_t dil);
int honk_conv_same_f32(const float* x, const float* w, float* y, int64_t batch, int32_t c, int32_t h, int32_t w_,
                       int32_t dil, int32_t flip, void* workspace, size_t workspace_bytes, void* stream);
int honk_conv_same_wgrad_f32(const float* x, const float* dy, float* dw, int64_t batch, int32_t c, int32_t h,
                             int32_t w_, int32_t dil, void* workspace, size_t workspace_bytes, void* stream);

/* ---- MFCC front-end (AudioPreprocessor.compute_mfccs, utils/manage_audio.py:30-42) ---- */
/*
 * pcm [batch][samples] f32 -> out [batch][frames][n_dct] f32 (the [B,101,40] model
 * input for 1 s @ 16 kHz, hop 160, n_fft 480, 40 mels/DCT), where
 *   frames = 1 + (samples + 2*(n_fft/2) - n_fft) / hop
 * is the frame count of the centre-padded clip: 1 + samples/hop for even n_fft; for odd
 * n_fft the padded clip is one sample shorter, so one frame fewer where hop divides samples.
 * window [n_fft], mel_weights [n_mels][n_fft/2+1], dct [n_dct][n_mels] are the
 * librosa-0.6 Hann window / Slaney mel basis / DCT basis (device, f32).
 * Centre reflect padding, power spectrum, log of positive entries.  batch <= 65535;
 * batch == 0: HONK_OK (for a shape the call takes; the shape is checked first).  HONK_ERR_ARG: a null pointer, batch < 0, samples < 1, n_fft < 2,
 * hop < 1, n_mels < 1, n_dct < 1, samples <= n_fft/2; HONK_ERR_UNSUPPORTED: n_fft past the
 * VALU route's LDS plan.
 */
int honk_mfcc_f32(const float* pcm, int64_t batch, int32_t samples, const float* window, int32_t n_fft,
                  int32_t hop, const float* mel_weights, int32_t n_mels, const float* dct, int32_t n_dct,
                  float* out, void* stream);
/*
 * The route honk_mfcc_f32 / honk_pcen_f32 take for a shape (host-only: no GPU work, no
 * pointer but `plan` dereferenced).  The launches read the very function these report:
 *   HONK_FRONT_ROUTE_MFMA  frames <= 112, n_fft % 16 == 0, hop % 4 == 0 and the kernel's LDS
 *                          plan within 160 KiB: one workgroup per clip, the spectrum on the MFMA
 *   HONK_FRONT_ROUTE_VALU  every other shape (and every shape under HONK_MFCC_VALU=1 in the
 *                          environment): a direct DFT per (clip, 4 frames), LDS plan within 64 KiB
 * They return the status and honk_last_error reason the launch would give for the shape:
 * HONK_ERR_ARG (as above, and a null plan), HONK_ERR_UNSUPPORTED past the VALU route's LDS plan.
 */
#define HONK_FRONT_ROUTE_MFMA 1
#define HONK_FRONT_ROUTE_VALU 2
typedef struct honk_front_plan_t {
  int32_t route;     /* HONK_FRONT_ROUTE_*                                                   */
  int32_t frames;    /* 1 + (samples + 2*(n_fft/2) - n_fft) / hop                            */
  int32_t n_bins;    /* n_fft/2 + 1                                                          */
  int32_t launches;  /* kernels per call: 1, or 2 on PCEN's VALU route (energies, then scan) */
  int64_t lds_bytes; /* dynamic LDS of the main kernel; above 64 KiB the call opts in first  */
} honk_front_plan_t;
int honk_mfcc_plan(int32_t samples, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t n_dct,
                   honk_front_plan_t* plan);
int honk_pcen_plan(int32_t samples, int32_t n_fft, int32_t hop, int32_t n_mels, honk_front_plan_t* plan);
/*
 * The same front end over a long recording (the /listen serving path, server.py:99-112):
 * every window of `window` samples that starts at sample w * stride of the int16 recording
 * pcm_i16 [samples] (device; converted x * 2^-15 in fp32, exact).  The recording has
 *   W = samples < window ? 0 : 1 + (samples - window) / stride
 * windows; the call computes windows [first_window, first_window + n_windows) into
 * out [n_windows][1 + window/hop][n_dct] fp32, each as honk_mfcc_f32 would from its own
 * samples (reflect padding about the window's own bounds).  With stride % hop == 0 the
 * frames whose n_fft span lies inside a window are frames of the recording: each is
 * computed once and written to every window that contains it; only the frames that cross a
 * window edge (0, 1, 99, 100 of the 101 at n_fft 480 / hop 160) are per window.  Otherwise
 * every frame is computed per window (no sharing, still no host slicing).  A frame's
 * n_dct values are a function of its n_fft samples alone (fixed summation order, no
 * floating-point atomics): ranges, chunks and shifted recordings agree bit for bit.
 *
 * honk_mfcc_windows_plan (host-only, no GPU work) fills the counts for a range and the
 * workspace size.  honk_mfcc_windows_i16 only enqueues on `stream` (no synchronisation,
 * no allocation: capturable).  HONK_ERR_ARG: a null pointer, a negative count, stride < 1,
 * window <= n_fft/2, a range past W; HONK_ERR_WORKSPACE: a short workspace;
 * HONK_ERR_UNSUPPORTED (reason in honk_last_error): n_fft or hop not a multiple of 16,
 * more than 128 mel bands, a shape past the kernel's LDS plan -- run honk_mfcc_f32 on the
 * windows then.  n_windows == 0: HONK_OK, nothing enqueued.
 */
typedef struct honk_mfcc_windows_plan_t {
  int64_t windows;         /* W of the whole recording                                   */
  int64_t shared_frames;   /* frames of the range computed once for all their windows    */
  int64_t edge_frames;     /* frames of the range computed per window (shared route)     */
  int64_t frames_computed; /* their sum; n_windows * frames on the unshared route        */
  int64_t workspace_bytes;
  int32_t shared;          /* 1: the shared route (stride % hop == 0), 0: per window     */
  int32_t frames;          /* 1 + window / hop                                           */
} honk_mfcc_windows_plan_t;
int honk_mfcc_windows_plan(int64_t samples, int32_t window, int32_t stride, int32_t n_fft, int32_t hop,
                           int64_t first_window, int64_t n_windows, honk_mfcc_windows_plan_t* plan);
int honk_mfcc_windows_i16(const int16_t* pcm_i16, int64_t samples, int32_t window, int32_t stride,
                          int64_t first_window, int64_t n_windows, const float* window_tbl, int32_t n_fft,
                          int32_t hop, const float* mel_weights, int32_t n_mels, const float* dct, int32_t n_dct,
                          float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- PCEN front-end (AudioPreprocessor.compute_pcen, utils/manage_audio.py:28,44-47) ---- */
/*
 * Per-channel energy normalisation (Wang et al. 2017), PARITY UNPINNED: the reference's
 * `pcen` package is not available, so this is the published algorithm and the defaults
 * below restate that package as best they can be without it.  For each clip of
 * pcm [batch][samples] f32, with honk_mfcc_f32's STFT (centre reflect padding, the
 * caller's window [n_fft] and mel_weights [n_mels][n_fft/2+1], device, f32):
 *   E[t][m] = sum_k mel_weights[m][k] * |X_t[k]|^power      power 1 (magnitude) or 2
 *   M[0] = E[0];  M[t] = (1 - s) M[t-1] + s E[t]            per band, reset for every clip
 *   out[t][m] = (E / (M + eps)^alpha + delta)^r - delta^r
 * out [batch][frames][n_mels] f32 (frames as honk_mfcc_f32's); no DCT.  The smoother starts
 * at M[0] = E[0] (HONK_PCEN_INIT_FIRST_FRAME, the only initial state built); zero energy
 * gives exactly 0.
 * params == NULL: the HONK_PCEN_* defaults.  Only enqueues on `stream` (no synchronisation,
 * no allocation, no workspace: capturable); batch <= 65535 per call; batch == 0: HONK_OK
 * (the shape and the parameters are checked first).
 * One launch when frames <= 112, n_fft % 16 == 0, hop % 4 == 0 and the LDS plan fits (the
 * MFMA MFCC kernel's shapes), else two (mel energies into out, then a segmented scan in
 * place); HONK_MFCC_VALU=1 in the environment forces the latter; honk_pcen_plan (above)
 * reports which.  HONK_ERR_ARG: a null pointer, samples <= n_fft/2, s outside (0, 1],
 * eps <= 0, alpha < 0, delta < 0, r <= 0, power not 1 or 2, a non-finite parameter;
 * HONK_ERR_UNSUPPORTED: n_fft past the two-launch route's LDS plan as well.
 */
#define HONK_PCEN_EPS 1e-6f
#define HONK_PCEN_S 0.025f
#define HONK_PCEN_ALPHA 0.98f
#define HONK_PCEN_DELTA 2.0f
#define HONK_PCEN_R 0.5f
#define HONK_PCEN_POWER 1
#define HONK_PCEN_INIT_FIRST_FRAME 1 /* M[0] = E[0] */
typedef struct { float eps, s, alpha, delta, r; int32_t power; } honk_pcen_params_t;
int honk_pcen_f32(const float* pcm, int64_t batch, int32_t samples, const float* window, int32_t n_fft,
                  int32_t hop, const float* mel_weights, int32_t n_mels,
                  const honk_pcen_params_t* params /* NULL = defaults */, float* out, void* stream);
/*
 * PCEN over a long recording (the /listen serving path of a PCEN-trained checkpoint): the
 * windows of honk_mfcc_windows_i16 -- W = samples < window ? 0 : 1 + (samples - window) / stride,
 * the range [first_window, first_window + n_windows), int16 -> x * 2^-15 -- into
 * out [n_windows][1 + window/hop][n_mels] fp32, each window as honk_pcen_f32 would give it from
 * its own samples: reflect padding about the window's own bounds, the smoother restarted at
 * M[0] = E[0] of the window's own frame 0.  With stride % hop == 0 the mel energies E of a frame
 * whose n_fft span lies inside a window are computed and stored once, whichever windows contain
 * it; the smoother and the compression then run per window (one workgroup each).  A frame's E
 * row is a function of its n_fft samples alone and a window's output of its E rows alone (fixed
 * summation order, no floating-point atomics, scan segments a function of (frames, n_mels)
 * only): ranges, chunks and shifted recordings agree bit for bit.
 *
 * honk_pcen_windows_plan (host-only) reports honk_mfcc_windows_plan's counts for the geometry
 * and this call's own workspace_bytes (the mel-range table; on the overlapping shared route
 * also frames_computed * n_mels floats of E).  honk_pcen_windows_i16 only enqueues on `stream`
 * (three launches; no synchronisation, no allocation: capturable); n_windows is not limited to
 * 65535.  Memory contract: the workspace's contents on entry are ignored and only
 * [0, workspace_bytes) of the plan is touched; out is fully written and nothing outside it;
 * pcm_i16 is never modified.
 * Status: every refusal of honk_mfcc_windows_i16 (HONK_ERR_ARG: a null pointer, a negative
 * count, stride < 1, window <= n_fft/2, a range past W, n_mels < 1; HONK_ERR_WORKSPACE: a short
 * workspace; HONK_ERR_UNSUPPORTED: n_fft or hop not a multiple of 16, more than 128 mel bands, a
 * shape past the frame kernel's LDS plan), every parameter refusal of honk_pcen_f32
 * (HONK_ERR_ARG, the same reasons), and HONK_ERR_UNSUPPORTED where a window's
 * [frames + 256 / n_mels][n_mels] tile is past 160 KiB of LDS -- run honk_pcen_f32 on the
 * windows then.  The shape and the parameters are checked first; n_windows == 0: HONK_OK,
 * nothing enqueued.
 */
int honk_pcen_windows_plan(int64_t samples, int32_t window, int32_t stride, int32_t n_fft, int32_t hop,
                           int32_t n_mels, int64_t first_window, int64_t n_windows,
                           honk_mfcc_windows_plan_t* plan);
int honk_pcen_windows_i16(const int16_t* pcm_i16, int64_t samples, int32_t window, int32_t stride,
                          int64_t first_window, int64_t n_windows, const float* window_tbl, int32_t n_fft,
                          int32_t hop, const float* mel_weights, int32_t n_mels,
                          const honk_pcen_params_t* params /* NULL = defaults */,
                          float* out /* [n_windows][1 + window/hop][n_mels] */,
                          void* workspace, size_t workspace_bytes, void* stream);
/*
 * The two calls above over a batch of recordings of ragged length in ONE call (a server that
 * listens to many streams at once: one front-end call, one forward and one download per tick).
 * The recordings lie in one device buffer pcm_i16 [total_samples]; the host array
 * offsets [n_rec + 1] (nondecreasing, 0 <= offsets[0], offsets[n_rec] <= total_samples) locates
 * them: recording r is pcm_i16[offsets[r] : offsets[r+1]], and samples outside
 * [offsets[0], offsets[n_rec]) belong to no recording and are never read.  Recording r has
 *   W_r = len_r < window ? 0 : 1 + (len_r - window) / stride
 * windows (0 for a short or empty one) and owns rows [window0[r], window0[r+1]) of
 * out [sum W_r][1 + window/hop][n_dct] (PCEN: n_mels), window0 the prefix sum of W_r.  Those
 * rows equal, bit for bit, what honk_mfcc_windows_i16 (honk_pcen_windows_i16) writes for that
 * recording alone with first_window = 0, n_windows = W_r: reflect padding about each window's
 * own bounds, each interior frame of a recording computed once for all of that recording's
 * windows, nothing read across a recording boundary, the same fixed-order per-frame arithmetic.
 *
 * One route (shared overlapping / shared gapped / unshared: a function of the geometry alone)
 * for the whole batch.  Segment tiles are laid out per recording, as the single-recording call
 * lays out that recording's, in recording order; edge tiles run over the batch's global window
 * index, so one edge tile holds windows of several recordings and a tick of many one-window
 * streams fills its edge tiles:
 *   tiles = sum_r seg_tiles_r + ceil(2 * sum W_r / groups_per_tile)     (unshared: the sum only)
 * A workgroup (in an edge tile: each group) finds its recording by a binary search over a
 * per-recording table in device memory: n_rec + 1 rows of six int64 (first segment tile, first
 * window, first shared-frame row, offsets[r], W_r, shared frames; the last row holds the totals).
 *
 * honk_*_segments_plan (host-only) validate offsets and fill the counts (sums over the
 * recordings of the single-recording plans), window0 [n_rec + 1] (may be NULL) and the table
 * (host memory of table_capacity bytes; NULL: sizes only; shorter than table_bytes:
 * HONK_ERR_WORKSPACE).  The caller copies the table to the device (table_dev).  The _i16 calls
 * take the host offsets again (the grid size; re-validated against total_samples) and only
 * enqueue on `stream`: no synchronisation, no allocation, no copy; capturable while pcm_i16,
 * table_dev, out and workspace keep their addresses and the offsets stay the same.  PCEN: on
 * the overlapping route the workspace holds [sum G_r][n_mels] shared E rows, then
 * [sum W_r][head + tail][n_mels] edge rows; stage 2 is one workgroup per global window.
 * n_rec == 0 or sum W_r == 0: HONK_OK, nothing enqueued (shape and parameters are checked first).
 * Status as the single-recording calls: HONK_ERR_ARG (a null pointer, a negative count, offsets
 * that decrease, are negative or run past total_samples, stride < 1, window <= n_fft/2, the PCEN
 * parameter refusals); HONK_ERR_UNSUPPORTED (n_fft or hop not a multiple of 16, more than 128
 * mel bands, the LDS plans, more than 2^31 - 1 tiles); HONK_ERR_WORKSPACE (a short workspace or
 * table).  Memory contract: the workspace's contents on entry are ignored and only
 * [0, workspace_bytes) of the plan is touched; out is fully written and nothing outside it;
 * pcm_i16 and table_dev are never modified.
 */
typedef struct honk_mfcc_segments_plan_t {
  int64_t windows;          /* sum W_r: rows of out                                        */
  int64_t shared_frames, edge_frames, frames_computed;   /* sums over the recordings       */
  int64_t tiles;            /* workgroups of the frame-tile kernel (formula above)         */
  int64_t workspace_bytes;  /* device workspace                                            */
  int64_t table_bytes;      /* the per-recording table: filled on the host, read on device */
  int32_t shared, frames;
} honk_mfcc_segments_plan_t;
int honk_mfcc_segments_plan(const int64_t* offsets, int64_t n_rec, int32_t window, int32_t stride,
                            int32_t n_fft, int32_t hop,
                            int64_t* window0 /* host [n_rec+1], may be NULL */,
                            void* table /* host, may be NULL: sizes only */, size_t table_capacity,
                            honk_mfcc_segments_plan_t* plan);
int honk_mfcc_segments_i16(const int16_t* pcm_i16, int64_t total_samples, const int64_t* offsets, int64_t n_rec,
                           const void* table_dev, size_t table_bytes, int32_t window, int32_t stride,
                           const float* window_tbl, int32_t n_fft, int32_t hop, const float* mel_weights,
                           int32_t n_mels, const float* dct, int32_t n_dct, float* out,
                           void* workspace, size_t workspace_bytes, void* stream);
int honk_pcen_segments_plan(const int64_t* offsets, int64_t n_rec, int32_t window, int32_t stride,
                            int32_t n_fft, int32_t hop, int32_t n_mels,
                            int64_t* window0 /* host [n_rec+1], may be NULL */,
                            void* table /* host, may be NULL: sizes only */, size_t table_capacity,
                            honk_mfcc_segments_plan_t* plan);
int honk_pcen_segments_i16(const int16_t* pcm_i16, int64_t total_samples, const int64_t* offsets, int64_t n_rec,
                           const void* table_dev, size_t table_bytes, int32_t window, int32_t stride,
                           const float* window_tbl, int32_t n_fft, int32_t hop, const float* mel_weights,
                           int32_t n_mels, const honk_pcen_params_t* params /* NULL = defaults */,
                           float* out /* [sum W_r][1 + window/hop][n_mels] */,
                           void* workspace, size_t workspace_bytes, void* stream);
/*
 * A stream bank: the segments calls for a server that listens tick after tick, with each
 * stream's unconsumed samples and the finished rows its next window reuses kept on the device
 * between ticks.  A tick takes only the NEW samples of the streams fed in it.
 *
 * Stream k has received x_k[0, N) and emitted E windows (window w = x_k[w stride, w stride +
 * window)).  A tick feeds c >= 0 samples: N' = N + c, E' = N' < window ? 0 : 1 + (N' - window) /
 * stride.  The tick's rows for the stream are, bit for bit, rows [E, E') of
 * honk_mfcc_windows_i16 (honk_pcen_windows_i16) on x_k[0, N') in a buffer of its own, whatever
 * the chunking, the other streams of the tick and the order of the slots: a frame's row is a
 * function of its own n_fft samples alone, in a fixed order, and the per-frame code is the same.
 *
 * Device state: n_slots * slot_bytes bytes of caller memory (state_dev), opaque to the caller;
 * a slot is [tail: at most window - 1 int16][two halves of cache_rows rows of row_floats
 * floats].  Host bookkeeping: one honk_bank_slot_t per slot, held by the caller; a slot is
 * opened (or reused) by zeroing its struct -- the device bytes need no initialisation.
 *   tail    samples in the slot: x_k[E stride, N) (stride > window: empty while E stride > N)
 *   skip    stride > window: the E stride - N samples still to come before the next window's
 *           start.  The CALLER drops them from later chunks before the upload and decrements
 *           skip; a tick that feeds samples to a slot with skip > 0 is refused
 *   cached  rows in the cache: 0 until the stream has emitted a window, then cache_rows
 *   parity  the cache half that holds them (a tick that completes a window writes the other)
 * The cache exists on the overlapping shared route only (stride % hop == 0 and q = stride / hop
 * <= fhi - flo, [flo, fhi] the interior frames): cache_rows = fhi - flo + 1 - q, row i the
 * interior frame flo + i of the stream's NEXT window (MFCC: its finished n_dct values; PCEN:
 * its n_mels mel energies before the smoother, which still restarts per window).  On the gapped
 * and unshared routes cache_rows = 0 and the bank saves only the upload.
 *
 * honk_stream_bank_plan (host-only): the slot geometry for row_floats floats per row (n_dct;
 * PCEN: n_mels); route 0 unshared, 1 overlapping, 2 gapped.
 *
 * honk_*_bank_tick_plan (host-only): slots [n_slots] the states before the tick, slot_ids
 * [n_fed] the fed slots (distinct, any order), chunk_offsets [n_fed + 1] (nondecreasing, >= 0)
 * locating each fed stream's new samples in chunks_dev.  Fills window0 [n_fed + 1] (rows
 * [window0[r], window0[r+1]) of out are fed stream r's; may be NULL), next [n_fed] (the fed
 * slots' states after the tick, for the caller to commit once the tick is enqueued; may be NULL),
 * the table (host memory of table_capacity bytes for the caller to copy to table_dev; NULL:
 * sizes only) and the counts.  A refused tick writes none of them.  A stream that completes
 * n >= 1 windows computes the frames jl >= flo + cached of its virtual window (n q in steady
 * state) and 2 (flo + frames - 1 - fhi) edge frames per window, and takes `cached` rows from
 * the cache: frames_computed and frames_reused are the sums.
 *
 * honk_*_bank_tick_i16 take the same slots / slot_ids / chunk_offsets again (re-validated) and
 * only enqueue on `stream`: no synchronisation, no device allocation, no copy by the host.
 * Launches: assemble "tail | chunk" per fed stream in the workspace; the frame-tile kernel
 * over the fed streams (a finished row the next window reuses also goes to the slot's other
 * cache half); PCEN's scan per window (cached rows, the tick's rows, the window's edge rows);
 * the cached rows' fan-out to out and their move to the other half; the new tails from the
 * workspace to the slots.  Within a launch no location is read by one workgroup and written by
 * another.  NOT meant for graph capture: the host bookkeeping, the table and the grid change
 * with every tick.
 * n_fed == 0 or no new sample: HONK_OK, nothing enqueued; new samples but no window: HONK_OK,
 * the tails advance (out may be NULL).  Status: HONK_ERR_ARG (a null pointer, a negative count,
 * offsets that decrease or are negative, a slot id out of range or fed twice, a slot state no
 * tick can have left, samples for a slot with skip > 0, and the shape / PCEN parameter refusals
 * of the segments calls); HONK_ERR_WORKSPACE (a short table, workspace or state_dev);
 * HONK_ERR_UNSUPPORTED (exactly the shapes the segments calls refuse).  The shape and the
 * parameters are checked first, before the counts are looked at: that includes the two refusals
 * no plan call above makes -- more than 128 mel bands (the MFCC plan calls take n_dct only) and
 * the frame-tile kernel's LDS plan with the epilogue's tiles and the group table
 * (honk_stream_bank_plan checks it without either).  So a tick with n_fed == 0 and every
 * pointer NULL returns the status every later tick of the shape would: a caller issues it once
 * when it builds the bank, and refuses the shape there.  Memory contract: out is fully written and nothing outside
 * it; only [0, workspace_bytes) of the workspace is touched and its contents on entry are
 * ignored; chunks_dev and table_dev are never modified; in state_dev only bytes of the fed
 * slots change.
 */
typedef struct honk_bank_slot_t { int32_t tail, cached, skip, parity; } honk_bank_slot_t;
typedef struct honk_stream_bank_plan_t {
  int64_t slot_bytes;       /* bytes of state_dev per slot                                  */
  int32_t tail_capacity;    /* window - 1                                                   */
  int32_t cache_rows;       /* fhi - flo + 1 - q on the overlapping route, else 0           */
  int32_t route, frames, row_floats, flo, fhi, q;
} honk_stream_bank_plan_t;
typedef struct honk_bank_tick_plan_t {
  int64_t windows;          /* sum over the fed streams: rows of out                        */
  int64_t frames_computed, frames_reused, edge_frames;
  int64_t tiles;            /* workgroups of the frame-tile kernel                          */
  int64_t workspace_bytes, table_bytes;
  int64_t samples_in;       /* chunk_offsets[n_fed] - chunk_offsets[0]                      */
} honk_bank_tick_plan_t;
int honk_stream_bank_plan(int32_t window, int32_t stride, int32_t n_fft, int32_t hop, int32_t row_floats,
                          honk_stream_bank_plan_t* plan);
int honk_mfcc_bank_tick_plan(const honk_bank_slot_t* slots, int64_t n_slots, const int64_t* slot_ids,
                             const int64_t* chunk_offsets, int64_t n_fed, int32_t window, int32_t stride,
                             int32_t n_fft, int32_t hop, int32_t n_dct,
                             int64_t* window0 /* host [n_fed+1], may be NULL */,
                             honk_bank_slot_t* next /* host [n_fed], may be NULL */,
                             void* table /* host, may be NULL: sizes only */, size_t table_capacity,
                             honk_bank_tick_plan_t* plan);
int honk_pcen_bank_tick_plan(const honk_bank_slot_t* slots, int64_t n_slots, const int64_t* slot_ids,
                             const int64_t* chunk_offsets, int64_t n_fed, int32_t window, int32_t stride,
                             int32_t n_fft, int32_t hop, int32_t n_mels,
                             int64_t* window0 /* host [n_fed+1], may be NULL */,
                             honk_bank_slot_t* next /* host [n_fed], may be NULL */,
                             void* table /* host, may be NULL: sizes only */, size_t table_capacity,
                             honk_bank_tick_plan_t* plan);
int honk_mfcc_bank_tick_i16(const int16_t* chunks_dev, const honk_bank_slot_t* slots, int64_t n_slots,
                            const int64_t* slot_ids, const int64_t* chunk_offsets, int64_t n_fed,
                            const void* table_dev, size_t table_bytes, void* state_dev, size_t state_bytes,
                            int32_t window, int32_t stride, const float* window_tbl, int32_t n_fft, int32_t hop,
                            const float* mel_weights, int32_t n_mels, const float* dct, int32_t n_dct,
                            float* out /* [windows][1 + window/hop][n_dct] */,
                            void* workspace, size_t workspace_bytes, void* stream);
int honk_pcen_bank_tick_i16(const int16_t* chunks_dev, const honk_bank_slot_t* slots, int64_t n_slots,
                            const int64_t* slot_ids, const int64_t* chunk_offsets, int64_t n_fed,
                            const void* table_dev, size_t table_bytes, void* state_dev, size_t state_bytes,
                            int32_t window, int32_t stride, const float* window_tbl, int32_t n_fft, int32_t hop,
                            const float* mel_weights, int32_t n_mels,
                            const honk_pcen_params_t* params /* NULL = defaults */,
                            float* out /* [windows][1 + window/hop][n_mels] */,
                            void* workspace, size_t workspace_bytes, void* stream);

/*
 * The last stage of /listen (ListenEndpoint.POST over TorchLabelService.label:
 * softmax -> np.argmax / np.max per window, then {label: summed prob} or the
 * command_tagging early exit per recording), on logits [n][n_labels] that stay on the
 * device.  Every pointer is device memory; the call only enqueues (rows, then segments:
 * two launches), needs no workspace and can be captured in a graph.
 *
 * Per window w:
 *   label[w] = the first index of the largest logit;
 *   prob[w]  = 1 / sum_j expf(z_j - max z) in fp32, summed in ascending j
 * -- independent of n and of the other windows, bit-equal from run to run.  A row whose
 * softmax is NaN in IEEE arithmetic (any NaN, any +inf, nothing above -inf) gives label 0,
 * prob NaN: what np.argmax / np.max return on torch's all-NaN softmax row.  A -inf among
 * finite logits is an ordinary zero term.
 *
 * Per segment s = windows [window0[s], window0[s+1]) (the layout of the segments calls'
 * and the bank ticks' window0, copied to the device by the caller):
 *   counts[s][l] = the number of its windows labelled l;
 *   sums[s][l]   = the sum of their prob in double;
 *   hit[s]       = the segment-relative index of the first window with label == keyword
 *                  && (double)prob >= min_prob, else -1 (always -1 for keyword < 0; NaN
 *                  compares false).
 * An empty segment gets zeros and -1.  A finite prob is at least 1 / n_labels >= 2^-6, hence
 * a multiple of 2^-29, and a sum of up to 2^23 of them is exact in double: sums does not
 * depend on the order of summation and equals the sequential host loop bit for bit (a NaN
 * prob makes its label's -- label 0's -- sum NaN).  A table entry is clamped to [0, n]
 * before use, so no table makes the call read outside label / prob; the results for a table
 * that decreases are unspecified.
 * segments == 0: window0_dev / sums / counts / hit may be NULL and are not touched.
 * n == 0: nothing per window is written (logits / label / prob may be NULL).
 * Status, decided on the host before anything is enqueued (honk_last_error has the text):
 * HONK_ERR_ARG (a negative count, a null pointer the counts require); HONK_ERR_UNSUPPORTED
 * (n_labels outside [1, HONK_LISTEN_MAX_LABELS], n above HONK_LISTEN_MAX_WINDOWS).
 * No float atomics; within a launch no location is written by one workgroup and read by
 * another.  Memory contract: label / prob [n], sums / counts [segments][n_labels] and hit
 * [segments] are fully written and nothing outside them; logits and window0_dev are never
 * modified.
 */
#define HONK_LISTEN_MAX_LABELS 64
#define HONK_LISTEN_MAX_WINDOWS ((int64_t)1 << 23)
int honk_listen_decide_f32(const float* logits, int64_t n, int32_t n_labels, const int64_t* window0_dev,
                           int64_t segments, int32_t keyword, double min_prob,
                           int32_t* label, float* prob /* [n] */,
                           double* sums, int32_t* counts /* [segments][n_labels] */,
                           int64_t* hit /* [segments] */, void* stream);

/* ---- training (data-parallel train(), utils/train.py:99-135) -------------------- */
/*
 * One torch.optim.SGD step (dampening 0) over a flat fp32 parameter bucket whose
 * gradients were summed across ranks; grad_scale = 1/world_size.  momentum_buf
 * (zero-initialised by the caller, re-zeroed when the reference re-creates its
 * optimizer at a schedule boundary, train.py:137-141) may be NULL iff momentum == 0.
 */
int honk_sgd_step_f32(float* params, const float* grads, float* momentum_buf, int64_t n, float lr,
                      float momentum, float weight_decay, float grad_scale, int32_t nesterov, void* stream);

/*
 * Training-mode 3x3 convolutions of the res block stack (dilation d, padding d, no
 * bias: model.py:94-98 -- d = 1 for res8/res26 and -narrow, d = 2**(i//3) for
 * res15 and res15-narrow), replacing the nn.Conv2d forward/backward that
 * utils/train.py:131-134 runs through autograd.  NCHW fp32, channels C in {19, 45};
 * w is the OIHW [C][C][3][3] conv weight; 1 <= dil <= 64.
 *   flip = 0: y = conv(x, w)                                (forward)
 *   flip = 1: y = conv(x, w'), w'[o][i][t] = w[i][o][8-t]   (input gradient: x = dy)
 */
int honk_conv3x3_f32(const float* x, const float* w, float* y, int64_t batch, int32_t c, int32_t h, int32_t w_,
                     int32_t dil, int32_t flip, void* stream);
/* Host-only: HONK_OK when honk_conv3x3_f32 / honk_conv3x3_wgrad_f32 cover (C, H, W, dil),
 * else the status (and honk_last_error text) those calls would return. */
int honk_conv3x3_check(int32_t c, int32_t h, int32_t w_, int32_t dil);
/*
 * Host-only: which kernels honk_conv3x3_f32 (forward / input gradient) and
 * honk_conv3x3_wgrad_f32 run `batch` clips of (C, H, W, dil) on, under the current
 * environment (HONK_TRAIN_CONV, HONK_WGRAD, HONK_TD_FIXED), as out[HONK_CONV3X3_PLAN_COUNT].
 * The launches read the same plan.  n_cus = 0: the current device's CU count.  A shape
 * honk_conv3x3_check refuses as unsupported gives HONK_OK with every entry 0 (the callers
 * run it on honk_conv_same_f32); HONK_ERR_ARG as honk_conv3x3_f32, and for batch < 1.
 * STATS: honk_conv3x3_stats_f32 / _tail_f32 take the shape (honk_conv3x3_stats_bytes > 0);
 * FOLD: honk_conv3x3_bn_fold_check.  A tile is TH rows of one dilation class of one clip at
 * full width, NBAND tiles per clip; a workgroup walks the tiles blockIdx.x, + GRID, ...
 */
#define HONK_CONV3X3_FAMILY_DMA 1  /* LDS-DMA staged fp32 MFMA: conv3x3d_kernel, wgrad3x3q/d_kernel */
#define HONK_CONV3X3_FAMILY_MFMA 2 /* register-staged fp32 MFMA: conv3x3m_kernel, wgrad3x3m_kernel  */
#define HONK_CONV3X3_FAMILY_VALU 3 /* conv3x3_kernel<C, NP>, wgrad3x3_kernel<C>                     */
#define HONK_CONV3X3_PLAN_OK 0            /* the dedicated kernels take the shape                  */
#define HONK_CONV3X3_PLAN_CONV_FAMILY 1
#define HONK_CONV3X3_PLAN_CONV_NP 2       /* VALU: output pixels per thread, else 0                */
#define HONK_CONV3X3_PLAN_CONV_FIXED 3    /* the compile-time 20-wide, 25-row instance             */
#define HONK_CONV3X3_PLAN_CONV_TH 4
#define HONK_CONV3X3_PLAN_CONV_NBAND 5
#define HONK_CONV3X3_PLAN_CONV_GRID 6
#define HONK_CONV3X3_PLAN_STATS 7
#define HONK_CONV3X3_PLAN_WGRAD_FAMILY 8
#define HONK_CONV3X3_PLAN_WGRAD_VARIANT 9 /* DMA: 'q', 'h' or 'd' (HONK_WGRAD), else 0             */
#define HONK_CONV3X3_PLAN_WGRAD_FIXED 10  /* the compile-time 20-wide, 17-row instance             */
#define HONK_CONV3X3_PLAN_WGRAD_TH 11
#define HONK_CONV3X3_PLAN_WGRAD_NBAND 12
#define HONK_CONV3X3_PLAN_WGRAD_GRID 13
#define HONK_CONV3X3_PLAN_FOLD 14
#define HONK_CONV3X3_PLAN_COUNT 16
int honk_conv3x3_plan(int64_t batch, int32_t c, int32_t h, int32_t w_, int32_t dil, int32_t n_cus, int32_t* out);
/* dw[o][i][ky][kx] = sum_{b,h,w} dy[b][o][h][w] * x[b][i][h+(ky-1)d][w+(kx-1)d] (zero padded);
 * deterministic: per-workgroup partials in the workspace, summed in a fixed order. */
size_t honk_conv3x3_wgrad_workspace_bytes(int64_t batch, int32_t c, int32_t h, int32_t w_, int32_t dil);
int honk_conv3x3_wgrad_f32(const float* x, const float* dy, float* dw, int64_t batch, int32_t c, int32_t h,
                           int32_t w_, int32_t dil, void* workspace, size_t workspace_bytes, void* stream);
/*
 * Train-mode BatchNorm2d(affine=False) (model.py:100 in training, nn.BatchNorm2d
 * semantics): y = (x - mean) * invstd with the biased batch variance over (B, H, W);
 * running stats (may both be NULL) <- (1 - momentum) running + momentum * batch
 * (unbiased variance); mean/invstd [C] are saved for the backward:
 * dx = invstd * (dy - mean(dy) - y * mean(dy * y)).  NCHW fp32, hw = H * W.
 */
size_t honk_bn_train_workspace_bytes(int64_t batch, int32_t c, int64_t hw);
/*
 * SyncBN (optional; honk_amd/syncbn.py): the caller all-reduces every
 * statistics-partials buffer across the data-parallel ranks before the BatchNorm that
 * finalises it, and sets the element-count scale k (the ranks' equal batches: k = world
 * size; thread-local, 1 by default) so the mean / variance / running statistics are the
 * whole job's.  honk_bn_partials_f32 writes the (sum a, sum a*b) partials ([c][S][2]
 * doubles, b NULL: a*a; S as honk_bn_train_workspace_bytes sizes) for a caller that reduces
 * them itself; honk_res_tail_bwd_mask*_f32 takes them with dil = -1.
 */
int honk_bn_count_scale(double k);
int honk_bn_partials_f32(const float* a, const float* b, void* part, size_t part_bytes, int64_t batch, int32_t c,
                         int64_t hw, void* stream);
int honk_bn_train_fwd_f32(const float* x, float* y, float* mean, float* invstd, float* running_mean,
                          float* running_var, int64_t batch, int32_t c, int64_t hw, float momentum, float eps,
                          void* workspace, size_t workspace_bytes, void* stream);
int honk_bn_train_bwd_f32(const float* dy, const float* y, const float* invstd, float* dx, int64_t batch,
                          int32_t c, int64_t hw, void* workspace, size_t workspace_bytes, void* stream);
/*
 * The res block tail around that BatchNorm, fused (model.py:111-118 in training:
 * x = relu(conv(x)); x = x + old_x on even layers; x = bn(x)), replacing the
 * relu / add / BatchNorm2d / threshold_backward / gradient-accumulation kernels
 * autograd runs for it (utils/train.py:131-134):
 *   forward:  s = relu(h) [+ old]  (old may be NULL; s written only when non-NULL),
 *             y = (s - mean) * invstd, batch statistics of s, running stats as above;
 *   backward: g = invstd * (gy - mean(gy) - y * mean(gy * y)) [+ gs]  (gs may be NULL:
 *             the gradient of s through its use as the next residual),
 *             gold = g (may be NULL), gh = (h > 0 ? g : 0).
 * Bit-identical to the unfused operations.  Workspace: honk_bn_train_workspace_bytes.
 */
int honk_res_tail_fwd_f32(const float* h, const float* old, float* s, float* y, float* mean, float* invstd,
                          float* running_mean, float* running_var, int64_t batch, int32_t c, int64_t hw,
                          float momentum, float eps, void* workspace, size_t workspace_bytes, void* stream);
int honk_res_tail_bwd_f32(const float* gy, const float* gs, const float* y, const float* invstd, const float* h,
                          float* gh, float* gold, int64_t batch, int32_t c, int64_t hw, void* workspace,
                          size_t workspace_bytes, void* stream);
/*
 * The tails' statistics computed in the producing conv's epilogue (the 19-map LDS-DMA
 * kernel's shapes: honk_conv3x3_stats_bytes > 0), so the tails skip their own pass:
 *   honk_conv3x3_stats_f32 = honk_conv3x3_f32 that also writes per-workgroup partial sums
 *   into `stats` -- mode 1 (forward conv, aux = old or NULL): of s = relu(y) [+ aux] and
 *   s*s; mode 2 (input-gradient conv, flip = 1, aux = the BN output y of the layer below):
 *   of the conv's output gy and gy*aux;
 *   honk_res_tail_fwd_part_f32 / honk_res_tail_bwd_part_f32 = honk_res_tail_fwd/bwd_f32
 *   taking those partials (mode 1 / mode 2 of the same shape; the backward also uses the
 *   buffer's tail as scratch).  Per-lane fp32 sums, then double in a fixed order: the
 *   statistics agree with the two-pass tails to fp32 rounding (not bit for bit).
 */
/*
 * The forward conv of a res block with the tail's elementwise head in its epilogue (the
 * statistics epilogue's shapes): s = relu(conv(x, w)) [+ old] is written instead of the
 * conv output (NCHW, as x), the ReLU's backward mask as one 32-bit word per pixel
 * (mask[b][h][w] bit o = !(conv[b][o][h][w] <= 0): NaN counts as > 0, as in torch's
 * threshold_backward; these shapes have c <= 20), and the statistics
 * of s as honk_conv3x3_stats_f32 mode 1.  Then honk_res_tail_fwd_s_f32 makes
 * y = BatchNorm_train(s) from s alone, and honk_res_tail_bwd_mask_f32 is
 * honk_res_tail_bwd_part_f32 with the mask in place of the conv output: the tails read
 * neither the conv output nor old, and write no separate s.  Same fp32 operations as the
 * unfused tails (bit-identical given the same statistics).
 */
int honk_conv3x3_tail_f32(const float* x, const float* w, float* s, uint32_t* mask, int64_t batch, int32_t c,
                          int32_t h, int32_t w_, int32_t dil, const float* old, void* stats, size_t stats_bytes,
                          void* stream);
int honk_res_tail_fwd_s_f32(const float* s, float* y, float* mean, float* invstd, float* running_mean,
                            float* running_var, const void* stats, int64_t batch, int32_t c, int32_t hh, int32_t ww,
                            int32_t dil, float momentum, float eps, void* stream);
/* dil >= 1: `stats` = the input-gradient conv's partials (honk_conv3x3_stats_f32 mode 2 at
 * dilation dil); dil = 0: `stats` is a workspace of honk_bn_train_workspace_bytes(batch, c,
 * hh * ww) and the statistics are summed here (a block whose output feeds no conv);
 * dil = -1: that workspace already holds honk_bn_partials_f32(gy, y) (SyncBN). */
int honk_res_tail_bwd_mask_f32(const float* gy, const float* gs, const float* y, const float* invstd,
                               const uint32_t* mask, float* gh, float* gold, int64_t batch, int32_t c,
                               int32_t hh, int32_t ww, int32_t dil, void* stats, size_t stats_bytes, void* stream);
size_t honk_conv3x3_stats_bytes(int64_t batch, int32_t c, int32_t h, int32_t w_, int32_t dil);
int honk_conv3x3_stats_f32(const float* x, const float* w, float* y, int64_t batch, int32_t c, int32_t h,
                           int32_t w_, int32_t dil, int32_t flip, int32_t mode, const float* aux, void* stats,
                           size_t stats_bytes, void* stream);
/*
 * The train BatchNorm of a res block folded into the next conv (res26-narrow's C5 step:
 * one HBM pass less per block -- the tail writes no y).  honk_res_tail_fwd_s_f32 with
 * y = NULL computes only mean / invstd / the running statistics; the consumers of y then
 * take that block's s with its (fold_mean, fold_invstd) and make y = (s - mean) * invstd
 * where they read it, tail_fwd's fp32 expression (bit-identical to the materialized y):
 *   honk_conv3x3_tail_bn_f32 / honk_conv3x3_stats_bn_f32 mode 1 -- the forward conv's
 *   input x (its staged tile, in LDS; the conv's zero padding stays zero);
 *   honk_conv3x3_stats_bn_f32 mode 2 -- the input-gradient conv's aux;
 *   honk_conv3x3_wgrad_bn_f32 -- the weight-gradient conv's x;
 *   honk_res_tail_bwd_mask_bn_f32 -- the tail backward's y (s = that tail's s, mean its
 *   mean; dil >= 1 only: a folded block always feeds an input-gradient conv).
 * The NULL-fold forms are the entry points above.  honk_conv3x3_bn_fold_check: HONK_OK when
 * the shape has all four (the statistics epilogue's shapes whose weight gradient runs on
 * the LDS-DMA kernels).  Replaces no reference call: the reference's bn (model.py:117-118)
 * is one module the drop-in keeps; this is the same arithmetic in a different kernel.
 */
int honk_conv3x3_bn_fold_check(int64_t batch, int32_t c, int32_t h, int32_t w_, int32_t dil);
int honk_conv3x3_tail_bn_f32(const float* x, const float* w, float* s, uint32_t* mask, int64_t batch, int32_t c,
                             int32_t h, int32_t w_, int32_t dil, const float* old, const float* fold_mean,
                             const float* fold_invstd, void* stats, size_t stats_bytes, void* stream);
int honk_conv3x3_stats_bn_f32(const float* x, const float* w, float* y, int64_t batch, int32_t c, int32_t h,
                              int32_t w_, int32_t dil, int32_t flip, int32_t mode, const float* aux,
                              const float* fold_mean, const float* fold_invstd, void* stats, size_t stats_bytes,
                              void* stream);
int honk_conv3x3_wgrad_bn_f32(const float* x, const float* dy, float* dw, int64_t batch, int32_t c, int32_t h,
                              int32_t w_, int32_t dil, const float* fold_mean, const float* fold_invstd,
                              void* workspace, size_t ws_bytes, void* stream);
int honk_res_tail_bwd_mask_bn_f32(const float* gy, const float* gs, const float* s, const float* mean,
                                  const float* invstd, const uint32_t* mask, float* gh, float* gold, int64_t batch,
                                  int32_t c, int32_t hh, int32_t ww, int32_t dil, void* stats, size_t stats_bytes,
                                  void* stream);
int honk_res_tail_fwd_part_f32(const float* h, const float* old, float* s, float* y, float* mean, float* invstd,
                               float* running_mean, float* running_var, const void* stats, int64_t batch, int32_t c,
                               int32_t h_, int32_t w_, int32_t dil, float momentum, float eps, void* stream);
int honk_res_tail_bwd_part_f32(const float* gy, const float* gs, const float* y, const float* invstd, const float* h,
                               float* gh, float* gold, void* stats, int64_t batch, int32_t c, int32_t h_, int32_t w_,
                               int32_t dil, void* stream);
/*
 * The res stem in training (model.py:104-110 in training: y = relu(conv0(x)), then
 * AvgPool2d((ph, pw)) when the config has res_pool; ph = pw = 1 without pool),
 * replacing the conv0 / relu / avg_pool2d kernels autograd runs and their backward
 * (utils/train.py:131-134).  x [B][H][W] fp32 (the MFCC input, no gradient), w0 the
 * [C][1][3][3] conv0 weight, y / gy [B][C][H/ph][W/pw]; 1 <= C <= 64, (H+2)(W+2) <= 8192.
 * honk_res_stem_wgrad_f32: dw0 = d(sum gy * y)/d w0 (the ReLU mask recomputed from x),
 * deterministic (per-workgroup partials summed in a fixed order).
 */
int honk_res_stem_fwd_f32(const float* x, const float* w0, float* y, int64_t batch, int32_t c, int32_t h, int32_t w_,
                          int32_t ph, int32_t pw, void* stream);
size_t honk_res_stem_wgrad_workspace_bytes(int64_t batch, int32_t c);
int honk_res_stem_wgrad_f32(const float* x, const float* w0, const float* gy, float* dw0, int64_t batch, int32_t c,
                            int32_t h, int32_t w_, int32_t ph, int32_t pw, void* workspace, size_t workspace_bytes,
                            void* stream);

/*
 * The training step's head (utils/train.py:129-131 with model.py:119-121): the
 * spatial mean z[r] = sum_i x[r][i] / hw over rows r = (b, c) (x.view(B, C, -1) then
 * torch.mean(x, 2)) and its backward gx[r][i] = gz[r] / hw; nn.CrossEntropyLoss()
 * (mean reduction): *loss = mean_b (logsumexp(z_b) - z_b[labels_b]) (a label outside
 * [0, n) gives NaN), and dlogits = (softmax(z_b) - onehot(labels_b)) * (*grad_loss) / batch
 * (grad_loss: the device scalar upstream gradient).  Fixed-order reductions.
 */
int honk_spatial_mean_f32(const float* x, float* z, int64_t rows, int32_t hw, void* stream);
int honk_spatial_mean_bwd_f32(const float* gz, float* gx, int64_t rows, int32_t hw, void* stream);
int honk_cross_entropy_f32(const float* logits, const int64_t* labels, float* loss, int64_t batch, int32_t n,
                           void* stream);
int honk_cross_entropy_bwd_f32(const float* logits, const int64_t* labels, const float* grad_loss, float* dlogits,
                               int64_t batch, int32_t n, void* stream);

/*
 * Training-set audio augmentation (SpeechDataset.load_audio, utils/model.py:282-306,
 * with _timeshift_audio :264-270), the per-clip transform on a batch of PCM
 * audio/out [batch][len] (the clips right-padded to len); the random draws are the
 * caller's (honk_amd/augment.py draws them on the reference's `random` stream):
 *   v[i] = (flags & HONK_AUG_SILENCE) ? 0 : (0 <= i + shift < len ? audio[i + shift] : 0)
 *   out[i] = (flags & HONK_AUG_NOISE) ? clip(amp * noise[noise_off + i] + v[i], -1, 1) : v[i]
 * in float32 (product rounded, then the sum; NaN kept).  shift/noise_off/amp/flags are
 * [batch] device arrays; noise is the concatenated background-noise bank
 * [noise_len] (NULL iff noise_len == 0; reads outside it are 0).  batch <= 65535.
 */
#define HONK_AUG_SILENCE 1
#define HONK_AUG_NOISE 2
int honk_augment_f32(const float* audio, const float* noise, const int32_t* shift, const int64_t* noise_off,
                     const float* amp, const int32_t* flags, float* out, int64_t batch, int32_t len,
                     int64_t noise_len, void* stream);

/* ---- diagnostics --------------------------------------------------------------- */
const char* honk_last_error(void);
const char* honk_version(void);
/*
 * Per-launch timing of the dominant kernel (res block conv) with hipEvents
 * recorded on the launch stream.  enable=1 starts a window (clears it);
 * honk_timing_read synchronises the recorded events and returns the summed
 * kernel time (ms), the launch count and the summed algorithmic FLOP.
 */
int honk_timing_enable(int32_t enable);
int honk_timing_read(double* total_ms, int64_t* launches, double* flop);

#ifdef __cplusplus
}
#endif
#endif /* HONK_HIP_H */
