/* pfr_hip.h — C ABI of libpfr_hip.so: the MI355X (gfx950) kernels behind the feature-extractor hot path of
 * MarQuisCheshire/Pets-Face-Recognition (train step of the CNN backbone into the ArcFace head, and the
 * embedding cosine match / candR@K).
 *
 * The reference is 100 % Python on PyTorch and has NO FFI boundary of its own; every entry
 * point below therefore names the PyTorch call on the reference's path that it replaces (file:line relative
 * to the reference tree).  The reference-side binding a maintainer would add is the ctypes stub shown in
 * INTEGRATION.md (our own host code in pets-face-recognition_amd/_hip/lib.py is exactly that stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (the library never allocates, frees or retains);
 *   - tensors are NHWC ("channels last"), dense, channel count a multiple of 16 bytes / sizeof(element);
 *   - dtype: PFR_F32 = 0 (exact-f32 MFMA, the parity path), PFR_BF16 = 1 (bf16 in, f32 accumulate), PFR_I8 = 2 (match only);
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); all calls are asynchronous;
 *   - workspaces are supplied by the caller; their sizes come from the *_splits / *_blocks / *_mtile queries;
 *   - return value: 0 = ok, <0 = error (PFR_ERR_*), message via pfr_last_error() (thread-local);
 *   - no global mutable state; thread-safe per stream.
 */
#ifndef PFR_HIP_H
#define PFR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFR_F32 0
#define PFR_BF16 1
#define PFR_I8 2   /* int8 selection operand of the gallery match (pfr_quantize_rows_i8), int32 accumulate */
#define PFR_OK 0
#define PFR_ERR_ARG (-1)
#define PFR_ERR_HIP (-2)
#define PFR_ERR_UNSUPPORTED (-3)

typedef void* pfr_stream_t; /* hipStream_t */

const char* pfr_last_error(void);
int pfr_version(void);
int pfr_device_arch(char* buf, int buflen);
/* Run-time tuning knobs — ONE table (csrc/pfr_api.hip); the library itself reads NO environment variable.  For A/B sweeps inside one
 * process and for pinning a kernel choice.  Keys (default):
 *   "igemm_p" (1) persistent GEMM kernel 0 never / 1 heuristic / 2 whenever eligible;  "igemm_ptile" (-1) its tile 0:128x128 1:64x128
 *   2:128x64 3:64x64 (rows x couts);  "igemm_pkch" (8) its k-step in 16-byte chunks;  "igemm_ppf" (0) its prefetch variants;
 *   "igemm_tile" (-1) / "igemm_kch" (0) / "igemm_big" (1): tile, k-step and 8-wave tiles of the one-tile-per-workgroup kernel;
 *   "sconv" (1) streaming 1x1 kernel 0 / 1 heuristic / 2 whenever eligible;  "sconv3" (1) halo-staged 3x3 64->64 kernel;
 *   "bnb" (0) BatchNorm-backward sums in the data-gradient epilogue: 1 tile kernels, 2 streaming kernels (the engines set 2);
 *   "swgrad" (1), "wgrad_big" (0), "wgrad_tile" (-1), "wgrad_splits" (0), "wgrad9" (1: the 56x56 class, 2: every geometry), "wgrad9_slots" (256 workgroups per launch): weight gradients;
 *   "bnb_tile3" (0) with bnb = 2: the 3x3 / stride-1 data gradients on the 256-row tile kernel leave the BatchNorm-backward sums too;
 *   "slin" (1) streaming Linear kernel for K = 96 j (Swin): 0 off, 1 for M >= 65536 rows, 2 whenever eligible;
 *   "attn_mfma" (1) window attention on MFMA;  "match_order" (1) L2-blocked tile order of the persistent filter GEMM of the gallery match.
 *   "ln_rb" (4) LayerNorm forward, rows in flight per lane group for C <= 512: 4, 6 or 8.
 *   "pair_mem_order" (1) grid order of pfr_pair_mem_loss_fwd / _bwd: 0 anchor block fast, 1 the anchor blocks of one partner range on one XCD
 *   (the same bits either way; profiles/pair_memory.txt).
 * Results do not depend on the knobs (same accumulation order per kernel family; alternatives are pinned bit-for-bit or to the oracle by the
 * tests); statistics-partial granularity follows pfr_conv2d_mtile.  pfr_get_tuning reads a knob back. */
int pfr_set_tuning(const char* key, int value);
int pfr_get_tuning(const char* key, int* value);
/* bumped by every pfr_set_tuning call that CHANGES a knob: launch plans that baked a kernel choice in (statistics-partial granularity,
 * partial-row counts) are rebuilt by their owners when the epoch they were built under is over */
int pfr_tuning_epoch(void);
/* Launch identity for tests that force a kernel with the knobs above: the kernel that took the calling thread's LAST launch of the
 * convolution family (pfr_conv2d_fwd / _dgrad_* / pfr_gemm_act* / pfr_conv1x1_* / pfr_conv2d_wgrad; 0 before the first).  Host
 * bookkeeping only (a thread-local the launchers store just before they launch): no device work, dispatch never reads it.
 *   id = family << 24 | detail
 *   family 1 tile kernel (pfr_igemm.hip)      detail: bits 0-2 tile (rows x couts) 0:128x128 1:64x128 2:128x64 3:64x64 4:256x256 5:256x128,
 *                                                     bit 3 (8) 128-byte k-steps (KCH 8; clear: KCH 4), bit 4 (16) FAST (C a k-step multiple),
 *                                                     bit 5 (32) PRO (fused operand prologue), bit 6 (64) EPRE (operand-row epilogue),
 *                                                     bit 7 (128) BNB (BatchNorm-backward sums), bit 8 (256) parity-class data gradient
 *   family 2 persistent kernel (pfr_igemm_p.hip)      bits 0-2 tile 0..3 as above, bit 3 KCH 8, bit 4 lean epilogue, bit 8 parity classes
 *                                                     (only the lean path — bf16 output, whole tiles, no post-ops — has 128-byte k-steps: the
 *                                                     general kernel runs KCH 4 and reports bit 3 clear whatever "igemm_pkch" is)
 *   family 3 streaming 1x1 (pfr_sconv.hip)            bits 0-3 epilogue: 0 plain 1 join / accumulate 2 bias(+ReLU) 3 bias + residual,
 *                                                     4-8 the BatchNorm-backward forms; bit 4 statistics; bit 5 four-wave column slices
 *   family 4 halo-staged 3x3 (pfr_sconv3.hip), 5 halo-staged stem (pfr_sstem.hip):  bit 0 statistics, bit 1 inference epilogue
 *   family 6 streaming Linear (pfr_slin.hip)          bits 0-2 epilogue: 0 plain 1 bias 2 bias + residual 3 GELU 4 GELU backward; bits 4-11 panel
 *   family 7 weight-gradient tile (pfr_wgrad.hip)     bits 0-1 the "wgrad_tile" number (bit 0: 64 couts, bit 1: 64 k columns; clear: 128),
 *                                                     bit 2 fused prologue, bits 8-23 splits
 *   family 8 256x256 weight-gradient tile, 9 streaming 1x1 weight gradient, 10 halo-staged 3x3 weight gradient:  bits 8-23 slabs written
 *   family 11 match filter (pfr_match_scores_filter / _i8): bits 0-2 tile (0 or 4), bit 3 KCH 8, bit 4 (16) several tiles per workgroup,
 *                                                     bit 5 (32) L2-blocked tile order ("match_order"), bits 6-7 element type 0 f32 1 bf16
 *                                                     2 i8, bits 8-11 query tiles per super-step of the blocked order (0: linear order) */
int pfr_debug_last_conv_kernel(void);

/* C-side executor of a pre-built launch plan (csrc/pfr_plan.hip): the host keeps a step's fixed list of C-ABI calls (fixed device
 * pointers) in a plan and replays it with ONE call instead of one interpreter round trip per launch.  An entry is appended with
 * the index of the entry point's thunk (pfr_plan_thunk_index("pfr_conv2d_fwd"), -1: not plannable) and its arguments as flat
 * 64-bit slots in declaration order WITHOUT the trailing stream (pointers / integers as such, floats as IEEE-754 bits).
 * kind: 0 launch on main | 1 launch on side | 2 fork (record event ev on main, side waits) | 3 record ev on side | 4 main waits
 * for ev | 5 as 4 but only when hook_stops == 1 (2: the hook synchronises with the side stream itself) | 6 hook stop (ev = user tag).  pfr_plan_run(begin, end <0 = all) returns -1 at the
 * end, the index of a kind-6 entry when hook_stops and it reached one (resume at index + 1), <= -2 on error. */
int pfr_plan_thunk_index(const char* name);
void* pfr_plan_create(int n_events);
int pfr_plan_destroy(void* plan);
int pfr_plan_append(void* plan, int kind, int thunk, int ev, const unsigned long long* args, int nargs);
int pfr_plan_size(void* plan);
int pfr_plan_run(void* plan, int begin, int end, pfr_stream_t main_stream, pfr_stream_t side_stream, int hook_stops);

/* ---- convolution / linear (implicit GEMM on MFMA) -------------------------------------------------------
 * pfr_conv2d_fwd replaces nn.Conv2d.forward / nn.Linear.forward / F.linear of the backbone and head
 * (torchvision resnet50 built at configs/dog_fe/fe_dogs_config.py:102-103; F.linear at
 * losses/large_margin.py:71) and — run over dy with flipped/transposed weights and idil_log2 = log2(stride) —
 * the autograd input gradient of the same ops.
 *   x [N][H][W][C], w [Cout][R][S][C], y [N*OH*OW][ldy] (ldy<=0 → Cout); ih = oh*stride - pad + r.
 *   bias [Cout] fp32 or NULL; residual [M][ldy] (y's dtype) or NULL: y = result + bias + residual;
 *   accumulate: y += result; out_relu: y = max(y,0)
 *   pro_scale/pro_shift [C] fp32 or NULL: operand is relu?(scale[c]*x + shift[c]) (fused BN-apply of the producer)
 *   stats_part or NULL: fp32 [ceil(M/mtile)][2][Cout] per-channel (mean, M2 = Σ(y-mean)²) of row groups of the stored y,
 *   mtile = pfr_conv2d_mtile(<the launch's geometry>, pro_scale != 0)  (input of pfr_bn_finalize; deterministic, no atomics):
 *   the m-tile height of the tile kernel that takes this geometry, half of it for the persistent kernel (one partial per wave row),
 *   or the rows of one workgroup's share for the streaming kernels (pfr_sconv.hip: a row range; pfr_sconv3.hip: 4x8-pixel patches
 *   in patch order) — pfr_bn_finalize only needs every group's row count, which is min(mtile, M - t*mtile) in all cases. */
int pfr_conv2d_mtile(int N, int H, int W, int C, int Cout, int R, int S, int stride, int pad, int OH, int OW, int dtype,
                     int out_dtype, int fused_prologue);
/* the same query for pfr_gemm_act_colstats (a launch with an activation epilogue always takes the tile kernel) */
int pfr_gemm_act_mtile(long M, int K, int N, int dtype);
int pfr_conv2d_fwd(const void* x, const void* w, void* y, int dtype, int out_dtype, int N, int H, int W, int C,
                   int Cout, int R, int S, int stride, int pad, int idil_log2, int OH, int OW, int ldy,
                   const float* bias, const void* residual, int accumulate, int out_relu, const float* pro_scale,
                   const float* pro_shift, int pro_relu, float* stats_part, pfr_stream_t stream);
/* data gradient of a block's first conv joined with the residual-branch gradient (autograd of torchvision
 * Bottleneck/BasicBlock `out += identity; out = relu(out)`): dx = dgrad(dy) + (mask ? res : 0).  dy [N][H][W][C], wt the
 * pfr_weight_dgrad_layout weights, dx / res [N][OH][OW][Cout]; res = gradient w.r.t. the block OUTPUT, res_mask = the ReLU
 * bit mask pfr_bn_act_mask wrote in forward ([N*OH*OW][Cout / (8 bf16 | 4 f32)] bytes); pad / idil_log2 as for the plain
 * data gradient through pfr_conv2d_fwd */
int pfr_conv2d_dgrad_join(const void* dy, const void* wt, void* dx, int dtype, int N, int H, int W, int C, int Cout, int R,
                          int S, int pad, int idil_log2, int OH, int OW, const void* res, const unsigned char* res_mask,
                          pfr_stream_t stream);

/* Data gradient that ALSO produces the BatchNorm-backward partial sums of the BN layer(s) whose OUTPUT gradient dx is (replaces
 * pfr_bn_bwd_reduce's pass over the gradient and the BN input; reference: autograd of nn.BatchNorm2d + ReLU after the conv,
 * torchvision resnet Bottleneck.forward).  part[t][0][c] = sum g*mask, part[t][1][c] = sum g*mask*xhat over the rows of m-tile t,
 * g = the value stored to dx, xhat = (x - mean)*invstd; mask = bn_mask bits ([M][Cout/KPACK] bytes of pfr_bn_act_mask) when given,
 * else scale*x + shift > 0.  bn_coef = [4][Cout] (mean, invstd, scale, shift rows, as pfr_bn_finalize writes them); bn2_* = an
 * optional second BN consuming the same gradient through the same bit mask (projection shortcut).  res/res_mask = the residual
 * join of pfr_conv2d_dgrad_join (both or neither), accumulate adds into dx.  pfr_conv2d_dgrad_bn_parts -> number of partial
 * rows per BN for the geometry (feed pfr_bn_bwd_finalize with it), or 0 when the fused form does not apply (run
 * pfr_bn_bwd_reduce instead).  With pfr_set_tuning("bnb", 2) (PFR_FUSE_BNB=2) the fused form is provided by the streaming kernels
 * only (1x1 / stride-1 geometries pfr_sconv.hip takes; parts = its row ranges): one BN, or two with the join; no accumulate, but `res`
 * without `res_mask` is a plain add and may alias dx (a gradient already accumulated there). */
int pfr_conv2d_dgrad_bn_parts(int dtype, int N, int H, int W, int C, int Cout, int R, int S, int idil_log2, int OH, int OW);
int pfr_conv2d_dgrad_bn(const void* dy, const void* wt, void* dx, int dtype, int N, int H, int W, int C, int Cout, int R, int S,
                        int pad, int idil_log2, int OH, int OW, const void* res, const unsigned char* res_mask, int accumulate,
                        const void* bn_x, const float* bn_coef, const unsigned char* bn_mask, float* bn_part, const void* bn2_x,
                        const float* bn2_coef, float* bn2_part, pfr_stream_t stream);

/* Main-branch data gradient of a block with a 1x1 / stride-2 projection shortcut: dx = dgrad(dy) + up2(res_compact) and the
 * BatchNorm-backward sums of the BN whose output gradient dx is.  res_compact [N][OH/2][OW/2][Cout] = the shortcut's gradient,
 * computed densely on its own grid (a plain pfr_conv2d_fwd over its dy with the pfr_weight_dgrad_layout weights), added at the
 * pixels with even (oh, ow).  Streaming form only (pfr_set_tuning("bnb", 2), pfr_conv2d_dgrad_bn_parts > 0, even OH / OW). */
int pfr_conv2d_dgrad_bn_sub(const void* dy, const void* wt, void* dx, int dtype, int N, int H, int W, int C, int Cout, int OH, int OW,
                            const void* res_compact, const void* bn_x, const float* bn_coef, const unsigned char* bn_mask,
                            float* bn_part, pfr_stream_t stream);

/* Recompute form of a bottleneck's last convolution (1x1, stride 1; torchvision Bottleneck.forward `out = relu(bn3(conv3(z)) + identity)`)
 * on the bf16 streaming kernel — the convolution output never reaches HBM: pfr_conv1x1_stats leaves only the BatchNorm partials (tile
 * height pfr_conv1x1_tail_mtile = pfr_conv2d_mtile of the geometry; 0: not taken, use pfr_conv2d_fwd + pfr_bn_act_mask), and after
 * pfr_bn_finalize pfr_conv1x1_bn_tail recomputes it and stores y = relu(a1*conv + b1 + (a2 ? a2*res + b2 : res)) with the ReLU bit mask
 * of pfr_bn_act_mask; bit-identical to the stored form (both round the convolution to bf16 first). */
int pfr_conv1x1_tail_mtile(int dtype, int N, int H, int W, int C, int Cout);
int pfr_conv1x1_stats(const void* x, const void* w, int dtype, int N, int H, int W, int C, int Cout, float* stats_part,
                      pfr_stream_t stream);
int pfr_conv1x1_bn_tail(const void* x, const void* w, void* y, unsigned char* mask, int dtype, int N, int H, int W, int C, int Cout,
                        const float* a1, const float* b1, const void* res, const float* a2, const float* b2, pfr_stream_t stream);

/* The two launches above with `flags` (streaming form with a bit mask only): 1 = dx is stored THROUGH bn_mask (dx = g*mask: every consumer
 * of a block-output gradient — the BN backward of the block's last BN, its projection BN, the residual join — reads it through that mask,
 * so they may then read it plainly); 2 = the first BN's input is not read: only sum g*mask is produced (row 1 of bn_part = 0; bn_x and
 * bn_coef may be NULL) — sum g*mask*xhat then comes out of pfr_bn3_bwd_coef. */
int pfr_conv2d_dgrad_bn_ex(const void* dy, const void* wt, void* dx, int dtype, int N, int H, int W, int C, int Cout, int R, int S,
                           int pad, int idil_log2, int OH, int OW, const void* res, const unsigned char* res_mask, int accumulate,
                           const void* bn_x, const float* bn_coef, const unsigned char* bn_mask, float* bn_part, const void* bn2_x,
                           const float* bn2_coef, float* bn2_part, int flags, pfr_stream_t stream);
int pfr_conv2d_dgrad_bn_sub_ex(const void* dy, const void* wt, void* dx, int dtype, int N, int H, int W, int C, int Cout, int OH, int OW,
                               const void* res_compact, const void* bn_x, const float* bn_coef, const unsigned char* bn_mask,
                               float* bn_part, int flags, pfr_stream_t stream);

/* Backward of a bottleneck's last 1x1 convolution + BatchNorm (autograd of `relu(bn3(conv3(z)) + shortcut)`, torchvision
 * Bottleneck.forward) WITHOUT the BatchNorm's input x = conv3(z) and without its gradient dx (csrc/pfr_bnfree.hip): BN backward is
 * linear, dx = A*G + B*(x - mean) + C0 per channel, and x - mean = (Z - zbar) W^T, so with G1 = G^T Z (pfr_conv2d_wgrad of the masked
 * gradient G [M][C] against Z [M][K]), G2 = Z^T Z, zsum = column sums of Z:
 *   pfr_bn3_bwd_coef:    dbeta = sum of part[t][0][:] (the partials pfr_conv2d_dgrad_bn[_ex] left), dgamma_c = invstd_c * sum_k W[c][k]
 *                        (G1[c][k] - dbeta_c zbar_k); coef [3][C] = A = gamma invstd, B = -gamma invstd^2 dgamma / M, C0 = -gamma invstd dbeta / M
 *   pfr_bn3_bwd_weights: dW = A*G1 + B*(W (G2 - M zbar zbar^T)) + C0 (x) (M zbar)   (fp32, += if accumulate);
 *                        wa_t [K][C] bf16 = A_c W[c][k] (data-gradient weight layout), S [K][K] bf16 = W^T diag(B) W, bias [K] = C0^T W - zbar S
 * and the data gradient is dZ = G wa_t^T + Z S + bias: pfr_conv2d_fwd(Z, S, bias) then pfr_conv2d_dgrad_bn(G, wa_t, res = that, no masks),
 * or — S == NULL: wa_t is then ONE concatenated tensor wcat [K][C + K], row k = [A*W column k | S row k] — a single
 * pfr_conv1x1_dgrad2_bn(G, Z, wcat, bias) launch over both row sources (bias added in fp32 inside the accumulators; BatchNorm-backward
 * sums of the BN dZ feeds as pfr_conv2d_dgrad_bn with a recomputed ReLU mask; pfr_conv1x1_dgrad2_bn_parts = partial rows, 0 = not taken).
 * W [C][K] (wdtype PFR_BF16 / PFR_F32) = the weights the FORWARD convolution multiplied with (the bf16 shadow on the bf16 path): every term
 * that reconstructs x = Z W^T must use the x that was actually normalised; count = M rows. */
int pfr_bn3_bwd_coef(const float* part, int nparts, const float* G1, const float* zsum, const void* W, int wdtype, const float* gamma,
                     const float* invstd, int C, int K, float count, float* dgamma, float* dbeta, float* coef, int accumulate,
                     pfr_stream_t stream);
int pfr_bn3_bwd_weights(const float* coef, const float* G1, const float* G2, const float* zsum, const void* W, int wdtype, int C, int K, float count,
                        float* dW, void* wa_t, void* S, float* bias, int accumulate, pfr_stream_t stream);
int pfr_conv1x1_dgrad2_bn_parts(int dtype, int N, int H, int W, int C1, int C2, int Cout);
int pfr_conv1x1_dgrad2_bn(const void* g, const void* z, const void* wcat, const float* bias, void* dx, int dtype, int N, int H, int W,
                          int C1, int C2, int Cout, const void* bn_x, const float* bn_coef, float* bn_part, pfr_stream_t stream);

/* G2 = X^T X [Q][Q] and the column sums of X [Q] in ONE streaming pass over X [M][Q] (bf16, Q = 64 | 128): the two forward-only inputs
 * of pfr_bn3_bwd_coef / pfr_bn3_bwd_weights.  out = Q*Q floats then Q floats; workspace = pfr_gram_ws_floats(M, Q) floats (0: geometry
 * not supported — pfr_conv2d_wgrad(x, x) + pfr_colsum give the same). */
/* batch statistics of x = Z W^T from pfr_gram_colsum's output for Z (no pass over x): mean_c = W[c] . zbar, var_c = W[c] (G2/M - zbar zbar^T)
 * W[c]^T; part = ONE (mean, M2) partial row [2][C] for pfr_bn_finalize(nparts = 1, rows_per_part = M).  W: the bf16 weights [C][K].
 * The subtraction cancels when a channel is nearly constant (|mean| >> std): the kernel bounds its own rounding error and, where that exceeds
 * 1 % of var + eps, stores 1 to *cancel_flag (may be NULL; host-visible memory lets the caller fall back to a statistics pass over x). */
int pfr_bn_stats_from_gram(const float* gram, const void* W, int dtype, int C, int K, float count, float* part, float eps, int* cancel_flag,
                           pfr_stream_t stream);
/* the same followed by pfr_bn_finalize(nparts = 1, rows_per_part = count) in one launch (results agree to the last bit or two; replaces torch.nn.BatchNorm2d's
 * training-mode statistics + running-stat update for a bottleneck's bn3: torchvision resnet.py Bottleneck.forward, third-party to /root/reference,
 * backbone built at configs/dog_fe/fe_dogs_config.py:102-103) */
int pfr_bn_finalize_from_gram(const float* gram, const void* W, int dtype, int C, int K, float count, const float* gamma, const float* beta,
                              float eps, float momentum, float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                              float* shift, int* cancel_flag, pfr_stream_t stream);
long pfr_gram_ws_floats(long M, int Q);
int pfr_gram_colsum(const void* x, int dtype, long M, int Q, float* out, float* workspace, pfr_stream_t stream);

/* pfr_conv2d_wgrad replaces the autograd weight gradient of nn.Conv2d / nn.Linear / F.linear:
 *   dw[co][r][s][c] (fp32) = scale * sum_m dy[m][co] * act(x)[...]  (+ dw if accumulate)
 * workspace: fp32 [pfr_conv2d_wgrad_splits(M,Cout,R*S*C)][Cout][R*S*C] (may be NULL when splits == 1). */
int pfr_conv2d_wgrad_splits(int M, int Cout, int KK);
int pfr_conv2d_wgrad(const void* x, const void* dy, float* dw, float* workspace, int dtype, int N, int H, int W, int C,
                     int Cout, int R, int S, int stride, int pad, int OH, int OW, int lddy, const float* pro_scale,
                     const float* pro_shift, int pro_relu, float scale, int accumulate, pfr_stream_t stream);

/* ---- layout / dtype helpers -------------------------------------------------------------------------- */
/* batch['x'] fp32 NCHW (data_loading/dataset.py:125) → NHWC compute dtype with Cp >= C zero-padded channels */
int pfr_nchw_to_nhwc(const float* x, void* y, int dtype, int N, int C, int H, int W, int Cp, pfr_stream_t stream);
int pfr_cast(const void* x, int src_dtype, void* y, int dst_dtype, size_t n, pfr_stream_t stream);
/* w [O][R][S][I] → wt [I][R][S][O], taps flipped: the weights pfr_conv2d_fwd needs to compute the data gradient */
int pfr_weight_dgrad_layout(const void* w, void* wt, int dtype, int O, int R, int S, int I, pfr_stream_t stream);
/* the same for n_layers convs in one launch; descs: DEVICE array of {const void* w; void* wt; int O, R, S, I;} (24 bytes each) */
int pfr_weight_dgrad_layout_batch(const void* descs, int n_layers, int dtype, pfr_stream_t stream);
int pfr_add(const void* a, const void* b, void* y, int dtype, size_t n, pfr_stream_t stream);
long pfr_colsum_ws_floats(long rows, int C); /* 0 for small row counts */
int pfr_colsum(const void* x, int dtype, long rows, int C, float* out, int accumulate, float* workspace, pfr_stream_t stream);
/* the same with the final merge deferred: pfr_colsum_partial leaves row-block partials in `workspace` (pfr_colsum_ws_floats floats,
 * one workspace per pending tensor); pfr_colsum_parts = how many partial rows that will be (0: too few rows, use pfr_colsum);
 * pfr_colsum_final_batch merges n partial sets in one launch.  descs: DEVICE array of {const float* part; float* out; int n; int C;
 * int accumulate; int mt; int rows; int pad} (40 bytes each); mt > 0: `part` holds the [n][2][C] m-tile statistics a GEMM epilogue
 * left (pfr_gemm_act_colstats, pfr_conv2d_fwd stats_part) for tiles of height mt over `rows` rows, and out = sum_t rows_t * mean_t */
int pfr_colsum_parts(int dtype, long rows, int C);
int pfr_colsum_partial(const void* x, int dtype, long rows, int C, float* workspace, pfr_stream_t stream);
int pfr_colsum_final_batch(const void* descs, int n, int max_C, pfr_stream_t stream);
int pfr_copy2d_f32(const float* src, int ld_src, float* dst, int ld_dst, long rows, int cols, float scale, int accumulate,
                   pfr_stream_t stream);

/* ---- BatchNorm2d (train: batch statistics, eps, momentum, unbiased running var — torchvision resnet) ---- */
int pfr_colreduce_blocks(int C, int dtype, long rows); /* partial rows written by pfr_bn_stats / pfr_bn_bwd_reduce */
int pfr_bn_stats(const void* x, int dtype, long rows, int C, float* part, pfr_stream_t stream);
long pfr_bn_stats_rows_per_part(int C, int dtype, long rows);
/* part: [nparts][2][C] = (mean_t, M2_t) of rows [t*rows_per_part, min(count, (t+1)*rows_per_part)) — written by
 * pfr_conv2d_fwd (rows_per_part = pfr_conv2d_mtile) or pfr_bn_stats (rows_per_part = pfr_bn_stats_rows_per_part). */
long pfr_bn_finalize_ws_floats(int nparts, int C); /* scratch floats for a parallel two-level merge (0: not needed) */
int pfr_bn_finalize(const float* part, int nparts, long rows_per_part, int C, float count, const float* gamma,
                    const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                    float* invstd, float* scale, float* shift, float* workspace, pfr_stream_t stream);
/* Inference embedder (Controller.validation_step / test_step, reference engine/controller.py:31-46, and the per-photo loop
 * of generate_tsv.py:233-251): eval-mode BatchNorm folded into the producing convolution, all layers in ONE launch.
 * descs: device array of ndesc records { const void* src; const float* gamma, *beta, *running_mean, *running_var;
 * void* wout; float* bout; long cout, k; float eps; int src_is_f32; } (80 bytes, natural alignment):
 * wout[co][k] = src[co][k] * gamma/sqrt(var+eps) in `dtype`, bout[co] = beta - mean*gamma/sqrt(var+eps) */
int pfr_fold_bn(const void* descs, int ndesc, int dtype, pfr_stream_t stream);
/* pfr_fold_bn that runs only when a parameter changed since the folded weights were made: a 64-bit position-weighted checksum of the
 * fp32 master buffer [n_master] and of every record's running statistics is taken on the device and compared with the previous
 * one; the master -> compute-dtype cast into `shadow` (may be NULL) and the fold exit at once when they agree.  state: 4 x 64-bit
 * device words owned by the caller, {0, ~0, 0, 0} before the first call; state[2] counts folds done, state[3] calls. */
int pfr_fold_bn_cached(const void* descs, int ndesc, int dtype, const float* master, size_t n_master, void* shadow,
                       unsigned long long* state, pfr_stream_t stream);
int pfr_bn_eval_coeff(int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float eps, float* scale, float* shift, pfr_stream_t stream);
/* y = relu?( a1*x1 + b1 (+ a2*x2 + b2 | + x2) ): BN apply, ReLU and the residual add of a bottleneck in one pass */
int pfr_bn_act(const void* x1, const float* a1, const float* b1, const void* x2, const float* a2, const float* b2, void* y,
               int dtype, long rows, int C, int relu, pfr_stream_t stream);
/* same, and (mask != NULL) also writes the sign of the pre-ReLU value as a bit mask: one byte per (row, 16-byte channel
 * chunk) = [rows][C / (8 bf16 | 4 f32)], bit e = (value of channel chunk*KP + e) > 0; the backward pass of a block's last
 * BN (relu(bn(x) + shortcut), torchvision Bottleneck.forward) reads this instead of the activation tensor */
int pfr_bn_act_mask(const void* x1, const float* a1, const float* b1, const void* x2, const float* a2, const float* b2,
                    void* y, unsigned char* mask, int dtype, long rows, int C, int relu, pfr_stream_t stream);
/* backward: g = dout * mask (mask_mode 0 none, 1: out > 0, 2: scale*x+shift > 0, 3: `out` is the bit mask of pfr_bn_act_mask);
 * reduce → partials of (Σg, Σg·x̂); finalize → dgamma, dbeta, coef[3][C]; apply → dx = coef0*g + coef1*x + coef2, gres = g */
int pfr_bn_bwd_reduce(const void* dout, const void* out, const void* x, const float* mean, const float* invstd,
                      const float* scale, const float* shift, int mask_mode, int dtype, long rows, int C, float* part,
                      pfr_stream_t stream);
int pfr_bn_bwd_finalize(const float* part, int nparts, int C, float count, const float* gamma, const float* mean,
                        const float* invstd, float* dgamma, float* dbeta, float* coef, int accumulate, pfr_stream_t stream);
int pfr_bn_bwd_apply(const void* dout, const void* out, const void* x, const float* coef, const float* scale,
                     const float* shift, int mask_mode, void* dx, void* gres, int dtype, long rows, int C,
                     pfr_stream_t stream);

/* ---- pooling (nn.MaxPool2d(3,2,1) fused with the stem's BN+ReLU; nn.AdaptiveAvgPool2d(1)) --------------- */
int pfr_bn_relu_maxpool_fwd(const void* x, const float* scale, const float* shift, void* y, uint8_t* idx, int dtype, int N,
                            int H, int W, int C, int relu, pfr_stream_t stream);
int pfr_maxpool_bwd(const void* dy, const uint8_t* idx, void* dz, int dtype, int N, int H, int W, int C, pfr_stream_t stream);
int pfr_avgpool_fwd(const void* x, void* y, int dtype, int N, int HW, int C, pfr_stream_t stream);
int pfr_avgpool_bwd(const void* dy, void* dx, int dtype, int N, int HW, int C, pfr_stream_t stream);

/* ---- ArcFace / CosFace head + (focal) cross-entropy (losses/large_margin.py:30-40,69-84; losses/losses.py:22-28) */
/* Space-to-depth form of the ResNet stem `conv1 = Conv2d(3, 64, 7, stride 2, padding 3)` (torchvision resnet, built at
 * configs/dog_fe/fe_dogs_config.py:102): the same sums as a 4x4 stride-1 pad-2 convolution over the half-resolution image
 * xs [N][H/2][W/2][Cp], channel (p*2+q)*C + c = x[c][2i+p][2j+q] (H, W even; Cp >= 4*C, zero padded), with weights
 * ws [Cout][4][4][Cp], ws[a][b][(p*2+q)*C + c] = w[2a+p-1][2b+q-1][c] (zero outside the 7x7 kernel).  Run it through
 * pfr_conv2d_fwd / pfr_conv2d_wgrad with R = S = 4, stride 1, pad 2, OH = H/2, OW = W/2.
 *   pfr_s2d_input : x fp32 NCHW -> xs (`dtype`)          pfr_s2d_weight: w fp32 [Cout][7][7][C] -> ws (`dtype`)
 *   pfr_s2d_wgrad : dws fp32 [Cout][4][4][Cp] -> dw fp32 [Cout][7][7][C] (+= if accumulate) */
int pfr_s2d_input(const float* x, void* y, int dtype, int N, int C, int H, int W, int Cp, pfr_stream_t stream);
int pfr_s2d_weight(const float* w, void* ws, int dtype, int Cout, int C, int Cp, pfr_stream_t stream);
int pfr_s2d_wgrad(const float* dws, float* dw, int Cout, int C, int Cp, int accumulate, pfr_stream_t stream);
/* y [cols][rows] = transpose of x [rows][cols] (the head's data gradient runs as a split-K GEMM over the class dimension:
 * autograd of F.linear in losses/large_margin.py:71, see losses/_head_hip.py) */
int pfr_transpose2d(const void* x, void* y, int dtype, int rows, int cols, pfr_stream_t stream);
/* match preparation (F.normalize of query / gallery embeddings, engine/controller.py:77-90 via similarity_f): one pass
 * over fp32 rows writes the L2-normalised row in bf16 (GEMM operand) and / or fp32 (exact re-scoring operand) */
int pfr_l2norm_dual(const float* x, void* xn_bf16, float* xn_f32, float* inv_norm, int rows, int D, float eps,
                    pfr_stream_t stream);
int pfr_l2norm_fwd(const void* x, int in_dtype, void* xn, void* xnT, int out_dtype, float* inv_norm, int rows, int D,
                   int ldt, float eps, pfr_stream_t stream);
int pfr_l2norm_bwd(const void* x, int in_dtype, const float* inv_norm, const float* dxn, void* dx, int out_dtype, int rows,
                   int D, int accumulate, pfr_stream_t stream);
/* mode 0 ArcFace hard margin, 1 ArcFace easy margin, 2 CosFace, 3 plain scaled cosine.
 * logits [B][C] fp32 or NULL, loss_rows [B] fp32 or NULL, dcos [B][ldc] (dcos_dtype) or NULL = grad_scale * d loss_row / d cos */
int pfr_margin_ce(const float* cosv, const int64_t* label, int B, int C, int ldc, int mode, float s, float m, float gamma,
                  float grad_scale, const float* grad_scale_dev, float* logits, float* loss_rows, void* dcos, int dcos_dtype,
                  pfr_stream_t stream);
/* standalone margin backward: dcos = s * dlogits (* dphi/dcos on the target column) */
int pfr_margin_bwd(const float* cosv, const int64_t* label, int B, int C, int ldc, int mode, float s, float m,
                   const float* dlogits, void* dcos, int dcos_dtype, pfr_stream_t stream);
int pfr_mean(const float* x, float* out, int n, pfr_stream_t stream);
/* pfr_margin_ce with the rest of `loss_kwargs` (losses/__init__.py:28-33) in the same single row kernel; all options off = pfr_margin_ce.
 *   alpha [C] fp32 or NULL: FocalLoss(alpha=True)'s `input = self.alpha * input` (losses/losses.py:23): the criterion runs on
 *     z = alpha * l (row maximum taken over z); `logits` stay the margin output l; dcos carries d loss / d l = alpha * dz.
 *   class_weight [C] fp32 or NULL, label_smoothing in [0, 1]: nn.CrossEntropyLoss(weight=, label_smoothing=) (F.cross_entropy):
 *     loss_row = (1-e) w_t (lse - l_t) + (e/C) (W lse - sum_c w_c l_c), W = sum_c w_c.  Exclusive with alpha and with gamma != 0.
 *   row_stats [B][4] fp32 or NULL: {lse, the row's gradient factor (focal f, or S = (1-e) w_t + (e/C) W), target margin logit l_t, w_t}:
 *     what pfr_alpha_grad and pfr_loss_reduce read.
 *   grad_scale_dev2: a second device scalar multiplied into the gradient scale (pfr_loss_reduce's 1 / denominator) or NULL. */
int pfr_margin_ce_ex(const float* cosv, const int64_t* label, int B, int C, int ldc, int mode, float s, float m, float gamma,
                     const float* alpha, const float* class_weight, float label_smoothing, float grad_scale,
                     const float* grad_scale_dev, const float* grad_scale_dev2, float* logits, float* loss_rows, float* row_stats,
                     void* dcos, int dcos_dtype, pfr_stream_t stream);
/* gradient of FocalLoss's alpha (autograd of `self.alpha * input`, losses/losses.py:23): dalpha[c] = grad_scale * (*grad_scale_dev) *
 * sum_i dz_ic * l_ic with dz recomputed from cos, alpha and pfr_margin_ce_ex's row_stats.  Column-wise, rows in a fixed order,
 * no atomics: bitwise reproducible. */
int pfr_alpha_grad(const float* cosv, const int64_t* label, const float* alpha, const float* row_stats, int B, int C, int ldc,
                   float s, float grad_scale, const float* grad_scale_dev, float* dalpha, pfr_stream_t stream);
/* the criterion's reduction (`.mean()` of losses/losses.py:28; F.cross_entropy's reduction): out_loss = sum(loss_rows) / d,
 * out_inv_denom (or NULL) = 1 / d; reduction 0: d = n, 1 ('sum'): d = 1, 2 (weighted 'mean'): d = sum_i row_stats[i][3] = sum_i w_{t_i} */
int pfr_loss_reduce(const float* loss_rows, const float* row_stats, int n, int reduction, float* out_loss, float* out_inv_denom,
                    pfr_stream_t stream);
/* Sub-centre heads (K centres per class, 1 <= K <= 16; weight row c*K + k, so a class's K sub-cosines are contiguous in a cosine row).
 * pfr_subcenter_pool replaces `cos, arg = cos_sub[:, :C*K].view(B, C, K).max(2)`: cos [B][ldc] fp32 with columns C..ldc-1 written as 0,
 *   arg [B][C] the LOWEST k that attains the maximum (strict > scan).  Columns C*K..ld_sub-1 of cos_sub are never read.
 *   label / count: both or neither; count [C*K] int32 is incremented (integer atomics) at label[b]*K + arg[b][label[b]] for every row:
 *   `count += torch.bincount(label*K + arg[range(B), label], minlength=C*K)`.
 * pfr_subcenter_scatter replaces the autograd of that max: dcos_sub[b][c*K+k] = (k == arg[b][c]) ? dcos[b][c] : 0 in the dtype of dcos
 *   (f32 or bf16), `torch.zeros(B, ld_sub).view(...).scatter_(2, arg[..., None], dcos[:, :C, None])`.  EVERY element of [B][ld_sub] is
 *   written, the pad columns as 0: no memset precedes it. */
int pfr_subcenter_pool(const float* cos_sub, int B, int C, int K, int ld_sub, float* cos, int ldc, uint8_t* arg, const int64_t* label,
                       int32_t* count, pfr_stream_t stream);
int pfr_subcenter_scatter(const void* dcos, int dtype, const uint8_t* arg, int B, int C, int K, int ldc, void* dcos_sub, int ld_sub,
                          pfr_stream_t stream);
/* Adaptive margins, kind 0 = AdaFace (Kim et al., CVPR 2022), 1 = CurricularFace (Huang et al., CVPR 2020).  Neither is in the
 * reference; as torch ops each is several B x C temporaries, a boolean mask, an indexed write and a scatter_ around the margin.
 * pfr_margin_prepare: one launch of one workgroup, fixed-order sums (no atomics: the same bits every launch), nothing read by the host.
 *   AdaFace replaces `a = norms.clip(1e-3, 100); mean = a.mean(); std = a.std(); batch_mean = t*mean + (1-t)*batch_mean` (likewise
 *   batch_std, left alone at B = 1); `k = (h * (a - batch_mean) / (batch_std + eps)).clip(-1, 1); g_ang = -m*k; g_add = m + m*k`:
 *   inv_norm [B] is what pfr_l2norm_fwd wrote (a = 1 / inv_norm), mean and the centred squares are two passes, state0 / state1 are the
 *   module's batch_mean / batch_std (updated in place when update != 0), `momentum` is t_alpha, row_margin [B][2] = {g_ang, g_add}
 *   from the buffers after the update, state_used [2] = {batch_mean, batch_std} as this call used them.
 *   CurricularFace replaces `t = momentum * cos[range(B), label].clamp(-1, 1).mean() + (1 - momentum) * t`: state0 is t (state1,
 *   inv_norm, row_margin unused, may be NULL), state_used = {t, 0}.  cos is the [B][ldc] fp32 class-cosine matrix (after sub-centre pooling).
 * pfr_margin_ce_adaptive: pfr_margin_ce_ex's row kernel (same logits / loss_rows / row_stats / grad_scale* / dcos conventions, plain and
 *   focal cross-entropy, class weights, label smoothing) with the margin kind as a compile-time switch; the learnable focal alpha is
 *   not available.  It reads row_margin (AdaFace) / state_used (CurricularFace) as pfr_margin_prepare wrote them for this step.
 *   AdaFace: c^ = clamp(cos, -1+eps, 1-eps) on every entry; target: theta' = clip(acos(c^) + g_ang, eps, pi - eps), l_t = s * (cos theta'
 *   - g_add), d l_t / d cos = s * sin theta' / sin theta; no gradient where a clamp or the clip is active.  `m` is unused.
 *   CurricularFace: cos clamped to [-1, 1]; target: ArcFace's hard margin (mode 0 of pfr_margin_ce); a negative with cos > cos(theta_t + m)
 *   is s * cos * (t + cos) with derivative s * (t + 2 cos).  `eps` is unused.
 * pfr_margin_bwd_adaptive: pfr_margin_bwd for these margins, dcos = s * dlogits * d l / d cos. */
int pfr_margin_prepare(int kind, const float* inv_norm, const float* cos, const int64_t* label, int B, int ldc, float m, float h,
                       float momentum, float eps, int update, float* state0, float* state1, float* row_margin, float* state_used,
                       pfr_stream_t stream);
int pfr_margin_ce_adaptive(const float* cos, const int64_t* label, int B, int C, int ldc, int kind, float s, float m, float eps,
                           float gamma, const float* class_weight, float label_smoothing, const float* row_margin,
                           const float* state_used, float grad_scale, const float* grad_scale_dev, const float* grad_scale_dev2,
                           float* logits, float* loss_rows, float* row_stats, void* dcos, int dcos_dtype, pfr_stream_t stream);
int pfr_margin_bwd_adaptive(const float* cos, const int64_t* label, int B, int C, int ldc, int kind, float s, float m, float eps,
                            const float* row_margin, const float* state_used, const float* dlogits, void* dcos, int dcos_dtype,
                            pfr_stream_t stream);
/* MagFace (Meng et al., CVPR 2021; not in the reference): the margin grows with the embedding's length a = clamp(|x|, l_a, u_a),
 * m = (u_m - l_m) / (u_a - l_a) * (a - l_a) + l_m, and g(a) = a / u_a^2 + 1 / a is a regulariser on the length.  The first head here
 * whose gradient has a radial part: d loss / d |x| flows through m on the target logit and through g.
 * pfr_magface_prepare: inv_norm [B] as pfr_l2norm_fwd wrote it (|x| = 1 / inv_norm, taken in fp32) -> row_margin [B][2] = {m, dm / d|x|}
 *   and row_reg [B][2] = {g(a), dg / d|x|}; both derivatives are 0 where the clamp is active (|x| < l_a or |x| > u_a; |x| equal to a
 *   bound counts as inside, as torch.clamp's autograd does).  Per-row arithmetic in fp64 rounded once, no sums, nothing read by the host.
 * pfr_margin_ce_magface: pfr_margin_ce_adaptive's row kernel (same logits / loss_rows / row_stats / grad_scale* / dcos conventions, plain
 *   and focal cross-entropy, class weights, label smoothing) with the MagFace margin: cos clamped to [-1, 1]; target
 *   phi = cos * cos m - sqrt(1 - cos^2) * sin m where cos > 0 (easy_margin != 0: else cos) or cos > cos(pi - m) (easy_margin == 0: else
 *   cos - m sin m), l_t = s * phi.  dnorm [B] fp32 or NULL = d(reduced loss) / d|x| with dcos's gradient scale:
 *   (d loss / d l_t) * s * (d phi / d m) * row_margin[i][1]  +  reg_scale * (*grad_scale_dev) * row_reg[i][1],
 *   d phi / d m = -sin(theta + m) where the margin is applied, else 0 (easy) or -(sin m + m cos m) (hard).  reg_scale is lambda_g / B
 *   for a mean reduction and lambda_g for 'sum'; row_reg may be NULL when reg_scale is 0.
 * pfr_margin_bwd_magface: pfr_margin_bwd_adaptive for this margin, dcos = s * dlogits * d l / d cos, and
 *   dnorm[i] = dlogits[i][t_i] * s * (d phi / d m) * row_margin[i][1] + reg_scale * (*reg_scale_dev or 1) * row_reg[i][1].
 * pfr_magface_loss: pfr_loss_reduce plus the regulariser in one launch of one workgroup, fixed order: out_reg = lambda_g * sum_i
 *   row_reg[i][0] / (1 for reduction 1 'sum', else n), out_loss = sum(loss_rows) / d + out_reg (d as pfr_loss_reduce).  loss_rows NULL:
 *   out_reg alone (out_loss / out_inv_denom may then be NULL).
 * pfr_l2norm_bwd_radial: pfr_l2norm_bwd plus the radial term, dx = inv_norm * (dxn - xn (xn . dxn)) + dnorm[row] * x[row] * inv_norm[row],
 *   in one pass; same dtypes and `accumulate`.  dnorm NULL: pfr_l2norm_bwd's kernel itself, the same bits. */
int pfr_magface_prepare(const float* inv_norm, int B, float l_a, float u_a, float l_m, float u_m, float* row_margin, float* row_reg,
                        pfr_stream_t stream);
int pfr_margin_ce_magface(const float* cos, const int64_t* label, int B, int C, int ldc, int easy_margin, float s, float gamma,
                          const float* class_weight, float label_smoothing, const float* row_margin, const float* row_reg,
                          float reg_scale, float grad_scale, const float* grad_scale_dev, const float* grad_scale_dev2, float* logits,
                          float* loss_rows, float* row_stats, void* dcos, int dcos_dtype, float* dnorm, pfr_stream_t stream);
int pfr_margin_bwd_magface(const float* cos, const int64_t* label, int B, int C, int ldc, int easy_margin, float s,
                           const float* row_margin, const float* row_reg, float reg_scale, const float* reg_scale_dev,
                           const float* dlogits, void* dcos, int dcos_dtype, float* dnorm, pfr_stream_t stream);
int pfr_magface_loss(const float* loss_rows, const float* row_stats, const float* row_reg, int n, int reduction, float lambda_g,
                     float* out_loss, float* out_inv_denom, float* out_reg, pfr_stream_t stream);
int pfr_l2norm_bwd_radial(const void* x, int in_dtype, const float* inv_norm, const float* dxn, const float* dnorm, void* dx,
                          int out_dtype, int rows, int D, int accumulate, pfr_stream_t stream);

/* ---- pair losses on the Gram matrix of the batch (csrc/pfr_pairloss.hip; not in the reference) ------------------------------
 * Embeddings e [B][D], labels y [B] (int64 of any sign, only compared for equality).  ê_i = e_i / max(|e_i|, eps) is what
 * pfr_l2norm_fwd wrote (`xn`, fp32 or bf16 = the compute dtype; int8 is not supported), s_ij = ê_i . ê_j with fp32 accumulation,
 * P(i) = {j != i : y_j = y_i}, N(i) = {j : y_j != y_i}; the diagonal belongs to neither set and has gradient 0.
 *   kind 0 'supcon' (Khosla et al. 2020, L_out), p0 = temperature tau (> 0), p1 unused.  Anchor i is valid when P(i) is not empty;
 *     l_i = log sum_{a != i} exp(s_ia / tau) - (1 / |P(i)|) sum_{p in P(i)} s_ip / tau,
 *     d l_i / d s_ia = (softmax_a - [a in P(i)] / |P(i)|) / tau for a != i.
 *   kind 1 'circle' (Sun et al. 2020, per anchor as pytorch-metric-learning does), p0 = m, p1 = gamma.  O_p = 1 + m, O_n = -m, D_p = 1 - m,
 *     D_n = m, alpha_p = max(0, O_p - s_p), alpha_n = max(0, s_n - O_n), both constants in the gradient.  Anchor i is valid when P(i) and
 *     N(i) are both non-empty;  z_i = LSE_{n in N(i)} gamma alpha_n (s_n - D_n) + LSE_{p in P(i)} (-gamma alpha_p (s_p - D_p)),
 *     l_i = softplus(z_i),  d l_i / d s_n = sigma(z_i) softmax_n gamma alpha_n,  d l_i / d s_p = -sigma(z_i) softmax_p gamma alpha_p.
 *   loss = (1 / A) sum over the valid anchors of l_i, A = their number; A = 0: loss = 0.0 exactly and an all-zero gradient.  Invalid
 *   anchors give no loss and no gradient; a log-sum-exp over an empty set never becomes a NaN; every log-sum-exp is max-subtracted
 *   (gamma = 256 works).  With W_ij = (1 / A) d l_i / d s_ij the gradient in normalised space is dê_r = sum_j (W_rj + W_jr) ê_j;
 *   pfr_l2norm_bwd takes it to e.  No floating-point atomics, the scalar is summed in a fixed order: the same bits every call.
 * pfr_pair_loss_fwd: one launch.  stats [B][4] fp32 = {lse_all, 1 / |P|, 1, valid} (supcon) or {lse_p, lse_n, sigma(z), valid}
 *   (circle), all 0 for an invalid anchor; ell [B] = l_i (0 where invalid); out [3] = {loss, 1 / A (0 when A = 0), A}.
 *   counter: ONE int32 of device memory that is 0 before the first launch and that the kernel leaves at 0 (the ticket of the
 *   last-workgroup reduction); launches that share it must be ordered on one stream.
 * pfr_pair_loss_bwd: one launch.  dxn [B][D] fp32 = grad_scale * (*grad_scale_dev or 1) * dê, every element written (plain stores).
 *   xnT [D][ldt] is ê transposed in the same dtype (pfr_l2norm_fwd's xnT), ldt a multiple of 32 >= B, columns B .. ldt-1 zero.  In bf16
 *   W_rj + W_jr is rounded to bf16 for the second product (fp32 accumulation); in fp32 nothing is rounded.
 * D is a multiple of 8, 8 <= D <= 1024; any B >= 1; ragged last tiles are masked. */
int pfr_pair_loss_fwd(const void* xn, int dtype, const int64_t* label, int B, int D, int kind, float p0, float p1, float* stats,
                      float* ell, float* out, int* counter, pfr_stream_t stream);
int pfr_pair_loss_bwd(const void* xn, const void* xnT, int dtype, int ldt, const int64_t* label, int B, int D, int kind, float p0,
                      float p1, const float* stats, const float* out, float grad_scale, const float* grad_scale_dev, float* dxn,
                      pfr_stream_t stream);

/* ---- pair losses with a cross-batch memory (csrc/pfr_pairmem.hip; Wang et al., CVPR 2020; not in the reference) --------------
 * The batch is that of pfr_pair_loss_fwd: ê [B][D] as pfr_l2norm_fwd wrote it, labels y [B].  The memory is a ring of past rows:
 * mem [M][D] in the same compute dtype (fp32 or bf16), labels mem_label [M] int64 and `count` in [0, M] live slots, which are always the
 * slots 0 .. count-1 (the ring fills from 0 and wraps only once it is full).  The partners of anchor i are the batch items j != i and
 * the live slots k:  P(i) = {j != i : y_j = y_i} u {k < count : ym_k = y_i},  N(i) = {j : y_j != y_i} u {k < count : ym_k != y_i}.
 * Logits, l_i, validity (supcon: P not empty; circle: P and N not empty) and loss = (1 / A) sum over the valid BATCH anchors of l_i
 * (A = 0: 0.0 exactly) are the formulas of pfr_pair_loss_fwd over these larger sets.  Memory items are never anchors and nothing flows
 * to them: with W_ij = (1 / A) d l_i / d s_ij,  dê_r = sum_{j in batch} (W_rj + W_jr) ê_j + sum_{k < count} W_rk m_k.
 *   Rows of mem at slots >= count may hold anything (NaN included): the kernels zero them in the operand, not only in the weight.  The
 *   transposed copy memT [D][ldm] has ldm a multiple of 32 >= M and the CALLER keeps it zero at columns >= count (pfr_pair_mem_push
 *   writes only live columns into a buffer that starts as zeros), as xnT's pad columns are.
 *   No floating-point atomics; every reduction has a fixed order: the same bits every call, whichever workgroup finishes last.
 *   D, dtype and the parameters are limited as for pfr_pair_loss_fwd; M is a multiple of 32 with 32 <= M < 2^24.  B <= M is what the
 *   push needs (a batch has to fit into the ring) and what the Python module enforces; the two loss kernels take any B.
 * The partner list is cut into tiles of 32: ceil(B / 32) batch tiles, then ceil(count / 32) memory tiles (a tile never holds both), and
 * the tile list into S contiguous splits, split s = tiles [s nt / S, (s + 1) nt / S); the grid is (anchor blocks of 32) x S.
 * pfr_pair_mem_splits: host arithmetic only.  -> the S that splits = 0 stands for: min(256 / anchor blocks, ceil(tiles / 4),
 *   64 MiB / (B D 4 bytes)), at least 1.  It sizes the workspace `ws` of both calls: forward S B 8 floats (partial states), backward
 *   S B D floats (slabs; the 64 MiB cap is the stated budget).  An explicit S needs a workspace of that S.
 * pfr_pair_mem_loss_fwd: one launch.  splits = 0: auto; an explicit S in [1, 4096] is honoured, also beyond the number of tiles (an
 *   empty split contributes the empty state (-inf, 0)).  S = 1: ws may be NULL.  Each workgroup writes the partial state of its 32
 *   anchors; the last workgroup (the integer ticket `counter`, as in pfr_pair_loss_fwd) merges the splits in split order and sums the
 *   scalar in a fixed order.  stats, ell, out: as pfr_pair_loss_fwd.
 * pfr_pair_mem_loss_bwd: dxn [B][D] fp32 = grad_scale * (*grad_scale_dev or 1) * dê, every element written with plain stores.  One
 *   launch when S = 1 (ws may be NULL); S > 1: every split writes a slab and a second small kernel on the same stream sums the slabs in
 *   split order.  In bf16 G (W_rj + W_jr, or W_rk) is rounded to bf16 for the second product (fp32 accumulation).
 * pfr_pair_mem_push: copies the B rows of xn to the slots (head + r) mod M: rows into mem, columns into memT, labels into mem_label.
 *   The caller advances head = (head + B) mod M and count = min(count + B, M).  It must run after the backward that reads the old ring. */
int pfr_pair_mem_splits(int B, int count, int D);
int pfr_pair_mem_loss_fwd(const void* xn, int dtype, const int64_t* label, int B, int D, const void* mem, const int64_t* mem_label, int M,
                          int count, int kind, float p0, float p1, int splits, float* ws, float* stats, float* ell, float* out,
                          int* counter, pfr_stream_t stream);
int pfr_pair_mem_loss_bwd(const void* xn, const void* xnT, int dtype, int ldt, const int64_t* label, int B, int D, const void* mem,
                          const void* memT, int ldm, const int64_t* mem_label, int M, int count, int kind, float p0, float p1,
                          const float* stats, const float* out, float grad_scale, const float* grad_scale_dev, int splits, float* ws,
                          float* dxn, pfr_stream_t stream);
int pfr_pair_mem_push(const void* xn, const int64_t* label, int B, int D, int dtype, void* mem, void* memT, int ldm, int64_t* mem_label,
                      int M, int head, pfr_stream_t stream);

/* ---- mined pair losses: batch-hard triplet and Multi-Similarity (csrc/pfr_pairmine.hip; not in the reference) ----------------
 * Operands, sets and reduction are those of pfr_pair_mem_loss_fwd: ê [B][D] as pfr_l2norm_fwd wrote it (fp32 or bf16), int64 labels, an
 * optional ring mem [M][D] / mem_label [M] with `count` live slots (mem = NULL, M = 0, count = 0: the batch alone), P(i) and N(i) over
 * the batch (diagonal excluded) plus the live slots.  Memory items are never anchors and nothing flows to them.  Anchor i is valid when
 * P(i) and N(i) are both non-empty; loss = (1 / A) sum over the valid batch anchors of l_i; A = 0: 0.0 exactly and an all-zero gradient.
 * Partners are numbered j for batch item j and B + k for slot k.
 *   Extremes (both kinds): s_p*(i) = min over P(i) of s_ij, s_n*(i) = max over N(i) of s_ij, each with its partner number.  Ties go to
 *   the smallest partner number, -0.0 = +0.0, and a pair whose score is a NaN counts for nothing: it is in neither set (the conventions
 *   of pfr_class_extremes).  These values, and every decision taken from them (which pair is the hardest, which pairs the miner keeps,
 *   whether the hinge is active), are CONSTANTS in the gradient.
 *   kind 2 'batch_hard' (Hermans et al. 2017, on cosine scores): params = {m >= 0, gamma >= 0, -, -}.  z_i = s_n* - s_p* + m;
 *     gamma = 0: l_i = max(0, z_i), active iff z_i > 0;  gamma > 0: l_i = softplus(gamma z_i) / gamma.  f_i = d l_i / d z_i;
 *     W_{i,n*} = +f_i / A, W_{i,p*} = -f_i / A, every other W is 0.
 *   kind 3 'multi_similarity' (Wang et al., CVPR 2019): params = {alpha > 0, beta > 0, base lambda, epsilon >= 0} (pytorch-metric-learning:
 *     2, 50, 0.5, 0.1).  Mining: negative n is kept iff s_in + epsilon > s_p*(i), positive p iff s_ip - epsilon < s_n*(i) (each sum rounded
 *     once in fp32).  L_p = log(1 + sum_{kept p} exp(-alpha (s_ip - lambda))), L_n = log(1 + sum_{kept n} exp(beta (s_in - lambda))),
 *     l_i = L_p / alpha + L_n / beta;  d l_i / d s_ip = -exp(-alpha (s_ip - lambda) - L_p),  d l_i / d s_in = exp(beta (s_in - lambda) - L_n)
 *     for kept pairs, 0 for the others.  Each log(1 + sum) is an online max-subtracted log-sum-exp that contains the element 0 (finite at
 *     beta = 256); an empty kept set gives 0.  Deviation from the published code, stated: the mean runs over the VALID anchors (this
 *     project's rule), not over the batch size with anchors skipped.
 *   The partner list, its tiles, the splits and pfr_pair_mined_splits (= pfr_pair_mem_splits; workspaces: forward S B 8 floats, backward
 *   S B D floats, multi_similarity only) are those of pfr_pair_mem_loss_fwd.  No floating-point atomics; the same bits every call,
 *   whichever workgroup finishes last.  Extremes, partner numbers, validity, kept counts and all of batch_hard do not depend on S at all
 *   (the merge of extremes is a total order); L_p, L_n and the multi_similarity gradient may differ between different S in the last
 *   bits, as the existing memory kernels' log-sum-exps and slab sums do.  D, dtype, M as there; any B >= 1; ragged tiles are masked; rows
 *   of mem at slots >= count may hold NaN and are zeroed in the operand.
 * pfr_pair_mined_fwd: params points to FOUR host floats, read during the call.  Launch 1, the extremes: the transposed 32 x 32 score tile,
 *   per-lane (min positive, its number, max negative, its number, |P|, |N|), merged over the waves in wave order and over the splits by the
 *   last workgroup (the integer ticket `counter`, contract of pfr_pair_loss_fwd); batch_hard ends here.  multi_similarity: launch 2 on the
 *   same stream scores the tiles again and accumulates the two gated log-sum-exps.
 *   stats [B][8] fp32: {s_p*, s_n*, number of p* (int32 bits), number of n* (int32 bits), L_p | z_i, L_n | f_i, kept pairs | 0, valid};
 *   an invalid anchor has the whole row 0 and both numbers -1.  ell [B] = l_i (0 where invalid); out [3] = {loss, 1 / A, A}.
 * pfr_pair_mined_bwd: dxn [B][D] fp32 = grad_scale * (*grad_scale_dev or 1) * dê, every element written with plain stores.
 *   multi_similarity: the dense form of pfr_pair_mem_loss_bwd (G_ij = W_ij + W_ji from the two stats rows and the recomputed score, the
 *   same pmn_keep decision as the forward; slabs and the ordered slab sum when S > 1; bf16 rounds G once).  batch_hard: sparse, no GEMM,
 *   xnT / memT / ws unused (may be NULL): row r = (f_r / A) (p[n*_r] - p[p*_r]) plus, for the anchors i in index order, +(f_i / A) ê_i
 *   where n*_i = r and -(f_i / A) ê_i where p*_i = r, fp32 throughout.  A stats row whose partner numbers are outside [0, B + count)
 *   contributes nothing: no address is formed from it. */
int pfr_pair_mined_splits(int B, int count, int D);
int pfr_pair_mined_fwd(const void* xn, int dtype, const int64_t* label, int B, int D, const void* mem, const int64_t* mem_label, int M,
                       int count, int kind, const float* params, int splits, float* ws, float* stats, float* ell, float* out,
                       int* counter, pfr_stream_t stream);
int pfr_pair_mined_bwd(const void* xn, const void* xnT, int dtype, int ldt, const int64_t* label, int B, int D, const void* mem,
                       const void* memT, int ldm, const int64_t* mem_label, int M, int count, int kind, const float* params,
                       const float* stats, const float* out, float grad_scale, const float* grad_scale_dev, int splits, float* ws,
                       float* dxn, pfr_stream_t stream);

/* ---- optimiser steps over flat fp32 master buffers (configs/dog_fe/fe_dogs_config.py:123-133; body_dog_fe.py:121-131) */
int pfr_sgd_step(float* p, const float* g, float* mom, void* shadow, int shadow_dtype, size_t n, float lr, float momentum,
                 float weight_decay, float grad_scale, int first_step, pfr_stream_t stream);
int pfr_adamw_step(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, size_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, pfr_stream_t stream);
/* the same steps with gradient clipping folded in: g' = clamp(g * grad_scale * (*clip_coef), ±clip_value).  clip_coef is a device
 * fp32 scalar (pfr_grad_norm's coefficient: torch.nn.utils.clip_grad_norm_'s `grads.mul_(clip_coef_clamped)`) or NULL = 1;
 * clip_value > 0 replaces torch.nn.utils.clip_grad_value_'s `grads.clamp_(-clip_value, clip_value)`, 0 = no clamp.
 * The gradient buffer is only read. */
int pfr_sgd_step_clip(float* p, const float* g, float* mom, void* shadow, int shadow_dtype, size_t n, float lr, float momentum,
                      float weight_decay, float grad_scale, int first_step, const float* clip_coef, float clip_value,
                      pfr_stream_t stream);
int pfr_adamw_step_clip(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, size_t n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                        const float* clip_coef, float clip_value, pfr_stream_t stream);
/* the _clip steps with a weight average folded in (clip_coef == NULL and clip_value == 0: no clipping): after the update, in the same
 * pass, avg <- lerp(avg, p_new, avg_weight), replacing torch.optim.swa_utils.AveragedModel.update_parameters' `torch._foreach_lerp_`
 * after optimizer.step().  avg_weight 1 copies (an AveragedModel's first update), 1 - decay is an EMA, 1 / (n_averaged + 1) SWA's
 * running mean.  torch.lerp's form: avg + w (p - avg) for w < 0.5, else p - (p - avg)(1 - w).  p, the optimizer state and the
 * shadow come out as from the _clip steps (without clipping: as from the plain steps), bit for bit.  avg: fp32 [n], laid out like p.
 * One launch each. */
int pfr_sgd_step_avg(float* p, const float* g, float* mom, void* shadow, int shadow_dtype, size_t n, float lr, float momentum,
                     float weight_decay, float grad_scale, int first_step, const float* clip_coef, float clip_value, float* avg,
                     float avg_weight, pfr_stream_t stream);
int pfr_adamw_step_avg(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, size_t n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                       const float* clip_coef, float clip_value, float* avg, float avg_weight, pfr_stream_t stream);
/* the same lerp on its own: avg <- lerp(avg, p, weight) over n floats (`avg.lerp_(p, weight)`; SWA's per-epoch update, parameters
 * outside a flat run, BatchNorm's cumulative moving average).  Any n, any 4-byte-aligned pointers (16-byte accesses where avg and
 * p share an alignment phase); nothing beyond n is read or written; no atomics. */
int pfr_weight_avg(float* avg, const float* p, size_t n, float weight, pfr_stream_t stream);
/* gradient norm over nseg dense fp32 segments (one per parameter), replacing torch.nn.utils.clip_grad_norm_'s
 * `torch._foreach_norm(grads, p)` + `vector_norm(stack(norms), p)` + clip coefficient, and PL's per-parameter grad_norm().
 * segs: device table [nseg] of {const float* ptr; int64 n; int64 first_chunk; int64 chunks} with chunks = ceil(n / chunk_elems),
 * chunk_elems = pfr_grad_norm_chunk_elems(), first chunks consecutive; chunk_seg: device int32 [nchunks] = segment of each chunk.
 * norm_p > 0: 1, 2, INFINITY, or any other p ((sum |x|^p)^(1/p), torch.linalg.vector_norm's ord).  ws: fp64 workspace
 * [nchunks + nseg].  out fp32 [nseg + 2]: the segment norms, the total over them, then min(1, max_norm / (total + 1e-6)).
 * Two launches, no atomics: bitwise reproducible; NaN / inf propagate as in torch. */
int pfr_grad_norm_chunk_elems(void);
int pfr_grad_norm(const void* segs, const int* chunk_seg, int nseg, long nchunks, float norm_p, float max_norm, double* ws,
                  float* out, pfr_stream_t stream);

/* ---- Partial FC: the margin head on a sampled subset of the class centres (csrc/pfr_pfc.hip; not in the reference) ----
 * pfr_pfc_sample: label int64 [B], score fp32 [C] (uniform draws in [0, 1)).  key[c] = 2.0 if c occurs in label, else score[c];
 *   index int32 [S] = the S classes with the largest key, ties towards the lower class id, ascending
 *   (= torch.sort(key, descending=True, stable=True).indices[:S].sort().values); local_label int64 [B] = position of label[b] in index
 *   (-1 for a label outside [0, C), which also flags no class).  Needs 1 <= S <= C and 1 <= B <= S.  ws: pfr_pfc_sample_ws_bytes(C)
 *   bytes of device memory (host arithmetic, no device work).  All work is queued on `stream`, nothing is read back; integer
 *   histograms and an ordered compaction: bitwise reproducible.
 * pfr_l2norm_gather_fwd: wn[s] = W[index[s]] / max(|W[index[s]]|, eps) for s < S, W fp32 [C][D], wn [Spad][D] in out_dtype with rows
 *   S .. Spad-1 zeroed, inv_norm fp32 [S]; wnT (NULL or [D][ldt], ldt >= Spad) the transposed copy with columns S .. Spad-1 zeroed.  The
 *   arithmetic is pfr_l2norm_fwd's for the same D and wnT: a gathered row has the bits of the same row of the full normalisation.
 * pfr_l2norm_gather_bwd: rows[s] = pfr_l2norm_bwd's result for row index[s] of W given dwn fp32 [>= S][D] and inv_norm [S].
 *   dense == 0: out is fp32 [S][D].  dense != 0: out is a fp32 [C][D] buffer the caller zeroed once, row index[s] receives rows[s], and
 *   the rows prev_index[0 .. prev_S) (the index of the call that last wrote this buffer, ascending; NULL / 0 for the first) that are not
 *   in index are set to zero in the same launch, so the buffer always holds exactly this call's rows.
 * pfr_sgd_step_rows: for r = index[s]: g = clamp(rows[s] * grad_scale * *clip_coef, +-clip_value) + weight_decay * p[r];
 *   mom[r] = momentum * mom[r] + g; p[r] -= lr * mom[r] (momentum == 0: p[r] -= lr * g, mom may be NULL).  p and mom fp32 [C][D], mom
 *   zero-initialised by the caller; clip_coef / clip_value / grad_scale as in pfr_sgd_step_clip.  Rows not listed are neither read nor
 *   written; index must not repeat a row. */
long pfr_pfc_sample_ws_bytes(long C);
int pfr_pfc_sample(const void* label, int B, const float* score, int C, int S, int* index, void* local_label, void* ws,
                   pfr_stream_t stream);
int pfr_l2norm_gather_fwd(const float* W, const int* index, void* wn, void* wnT, int out_dtype, float* inv_norm, int S, int Spad,
                          int C, int D, int ldt, float eps, pfr_stream_t stream);
int pfr_l2norm_gather_bwd(const float* W, const int* index, const float* inv_norm, const float* dwn, float* out, int S, int C, int D,
                          int dense, const int* prev_index, int prev_S, pfr_stream_t stream);
int pfr_sgd_step_rows(float* p, const int* index, const float* rows, float* mom, int S, int C, int D, float lr, float momentum,
                      float weight_decay, float grad_scale, const float* clip_coef, float clip_value, pfr_stream_t stream);

/* ---- Swin-T feature extractor (models/swin.py:8-241): LayerNorm (29,215), exact GELU (39-43), fused shifted-window
 * attention (101-135).  Linear layers and the Unfold+Linear patch merging (a stride-f conv) use pfr_conv2d_*. */
int pfr_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int dtype,
                      long rows, int C, float eps, pfr_stream_t stream);
int pfr_layernorm_bwd_blocks(long rows); /* part is fp32 [2][blocks][C]: dgamma partial rows, then dbeta partial rows (sum each half with pfr_colsum) */
int pfr_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                      const void* dres, void* dx, float* part, int dtype, long rows, int C, pfr_stream_t stream);
/* the same pass that also leaves the per-workgroup column sums of dx (dxsum_part [pfr_layernorm_bwd_blocks(rows)][C], may be NULL):
 * torch autograd computes the bias gradient of the nn.Linear / patch-merging layer in front of the LayerNorm as a separate
 * reduction over that gradient (models/swin.py:157-190 blocks, 84-99 PatchMerging); pfr_layernorm_bwd_dxsum_ok(dtype, C) = 1 when
 * the channel count takes the kernel that can do it */
int pfr_layernorm_bwd_dxsum(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                            const void* dres, void* dx, float* part, float* dxsum_part, int dtype, long rows, int C,
                            pfr_stream_t stream);
int pfr_layernorm_bwd_dxsum_ok(int dtype, int C);
int pfr_gelu_fwd(const void* x, void* y, int dtype, size_t n, pfr_stream_t stream);
int pfr_gelu_bwd(const void* x, const void* dy, void* dx, int dtype, size_t n, pfr_stream_t stream);
/* bias(+mask) table of one attention block: tab fp32 [4][64][64] (-inf outside w*w x w*w) followed by a second copy of the same
 * values in the MFMA kernels' access order (pfr_window_bias_table_floats = both; always allocate that many floats and pass the
 * buffer whole to pfr_window_attn_fwd / _bwd); variant 2*(last window row)+(last window column); built from the (2w-1)x(2w-1) relative-position table `pos` (models/swin.py:65-70,93-95,117-118) and the shifted-window
 * masks (create_mask, models/swin.py:49-62,86-90,122-124); rebuild whenever pos changed */
long pfr_window_bias_table_floats(int window);
int pfr_window_bias_table(const float* pos, float* tab, int window, int shift, pfr_stream_t stream);
/* the tables of n attention blocks in one launch; descs: DEVICE array of {const float* pos; float* tab; int window; int shift;}
 * (24 bytes each; window * window <= 64 is the caller's to check) */
int pfr_window_bias_table_batch(const void* descs, int n, pfr_stream_t stream);
/* qkv [B][H][W][3*heads*head_dim] (q|k|v, each (head, d)); pos: the TABLE built by pfr_window_bias_table;
 * shift = cyclic displacement (0 or w/2); out [B][H][W][heads*head_dim] */
int pfr_window_attn_fwd(const void* qkv, const float* pos, void* out, int dtype, int B, int H, int W, int heads, int head_dim,
                        int window, int shift, float scale, pfr_stream_t stream);
/* dpos_part: fp32 [B*(H/w)*(W/w)*heads][(2w-1)^2] per-workgroup partials of the table gradient (sum with pfr_colsum) */
int pfr_window_attn_bwd(const void* qkv, const float* pos, const void* dout, void* dqkv, float* dpos_part, int dtype, int B,
                        int H, int W, int heads, int head_dim, int window, int shift, float scale, pfr_stream_t stream);
int pfr_nhwc_to_nchw_f32(const float* x, float* y, int N, int C, int HW, int Cp, int accumulate, pfr_stream_t stream);

/* ---- embedding match: running top-K over gallery chunks (engine/controller.py:77-90,143-160; generate_tsv.py:91-125;
 * similarity_f = (cos+1)/2 at configs/dog_fe/fe_dogs_config.py:89-93).  Scores of a chunk come from pfr_conv2d_fwd
 * (plain GEMM of L2-normalised rows, fp32 out).  Order: score descending, ties → lower gallery index. */
long pfr_topk_state_bytes(int rows, int K);
int pfr_topk_reset(void* state, int rows, int K, pfr_stream_t stream);
/* scores [rows][ld] fp32, n valid columns, gallery index of column j = col0 + j; chunks must come in increasing col0.
 * self_idx [rows] int32 or NULL: gallery index to skip per query (all-vs-all evaluation excludes the query itself) */
int pfr_topk_update(const float* scores, int rows, int ld, int n, int col0, int K, void* state, const int* self_idx,
                    pfr_stream_t stream);
/* fused form for every chunk after the first (all running lists full): the match GEMM q[Q][D] x g[n][D]^T with the top-K
 * filter in its epilogue — a score is appended to query r's candidate list cand[r][0..cap) (u64 key<<32 | ~index) iff it
 * beats r's current K-th best; the fp32 score matrix is never written.  pfr_topk_merge then folds the candidates into
 * the running lists.  exclude_self: skip gallery index == query row.  Overflow of a candidate list sets bit 1 of
 * pfr_topk_flags: the caller must redo the match with pfr_topk_update. */
int pfr_match_scores_filter(const void* q, const void* g, int dtype, int Q, int n, int D, int col0, int K, void* state,
                            void* cand, int cap, int exclude_self, pfr_stream_t stream);
int pfr_topk_merge(const void* cand, int cap, int rows, int K, void* state, pfr_stream_t stream);
/* ---- int8 selection (match.cosine_topk(compute_dtype=torch.int8)): per-row scalar-quantised operands, exact int32 accumulation on
 * v_mfma_i32_32x32x32_i8, fp32 selection scores that feed the same running lists, filter, re-scoring and certificate as bf16.
 *   Quantiser, per row x[0..D):  x̂ = x · inv with inv = 1 / max(|x|_2, eps) (the arithmetic of pfr_l2norm_dual), or x̂ = x when
 *     normalize == 0;  m = max_i |x̂_i|;  r = 127.0f / m;  q_i = (int8) rintf(x̂_i · r) (round half to even);  s = m / 127.0f.
 *     When r is +inf (m == 0, or m so small that the quotient overflows) the row is all zero and s = 0.  Columns D .. ldq-1 are 0.
 *   Selection score of query row a and gallery row b:  score = ((float) acc · s_a) · s_b  with acc = Σ_i q_a,i · q_b,i accumulated
 *     exactly in int32 (the conversion to float rounds to nearest even; exact for Dp <= 1040), the two fp32 products in this order.
 *     pfr_match_scores_i8 and the filter epilogue of pfr_match_scores_filter_i8 compute it with the same operations: the same bits.
 * pfr_quantize_rows_i8: x [rows][D] fp32 (D % 4 == 0, D <= 2048) -> q [rows][ldq] int8 (ldq >= D, ldq % 4 == 0; the match needs
 *   ldq = Dp, a multiple of 128), scale [rows] fp32, and when non-NULL xn_f32 [rows][D] = x̂ and inv_norm [rows] = inv (normalize only). */
int pfr_quantize_rows_i8(const float* x, void* q, int ldq, float* scale, float* xn_f32, float* inv_norm, int rows, int D, int normalize,
                         float eps, pfr_stream_t stream);
/* selection scores of one gallery chunk: out [Q][ld] fp32 (n valid columns) = score(q row, g row) for q [Q][Dp], g [n][Dp] int8 rows of
 * pfr_quantize_rows_i8 with their scales q_scale [Q], g_scale [n] (g and g_scale point at the chunk's first row).  Dp % 128 == 0, <= 2048. */
int pfr_match_scores_i8(const void* q, const float* q_scale, const void* g, const float* g_scale, int Q, int n, int Dp, float* out, int ld,
                        pfr_stream_t stream);
/* pfr_match_scores_filter on the int8 operands above: a selection score is appended to query r's candidate list iff its key beats r's
 * current K-th best (exact: the comparison is on the score as defined, not on a bound of it). */
int pfr_match_scores_filter_i8(const void* q, const float* q_scale, const void* g, const float* g_scale, int Q, int n, int Dp, int col0,
                               int K, void* state, void* cand, int cap, int exclude_self, pfr_stream_t stream);
int pfr_topk_flags(const void* state, int rows, int K, int* out_host, pfr_stream_t stream);
int pfr_topk_finish(const void* state, int rows, int K, float* out_scores, int* out_idx, pfr_stream_t stream);
/* exact fp32 re-scoring of KC candidates per query, keeps the best K.  q: L2-normalised fp32 rows; g: L2-normalised fp32 rows (g_scale
 * NULL), or the RAW gallery rows with g_scale[i] = 1 / max(|g_i|, eps) (pfr_l2norm_dual's inv_norm output): the score is <q, g_i> * g_scale[i]
 * and no normalised fp32 copy of the gallery has to exist (2 GB less written per 1 M x 512 match) */
int pfr_topk_rescore(const float* q, const float* g, const float* g_scale, int rows, int D, const int* cand, int KC, int K,
                     float* out_scores, int* out_idx, pfr_stream_t stream);
/* the same, and the certificate of the two-precision match (the reference scores every pair in fp32 — utils/calc_scores.py's torch.mm — so a
 * reduced-precision candidate selection has to show that it lost nothing): cand_scores [rows][KC] = the selection scores pfr_topk_finish
 * returned with cand; cert [rows][2] fp32: cert[r][0] = max |fp32 score - selection score| over r's candidates, cert[r][1] = (K-th best
 * fp32 score) - (selection score of r's last candidate), +inf when the list holds every eligible gallery row.  A gallery row outside the list
 * can belong to r's exact top-K only if its selection error exceeds cert[r][1]; the host compares that gap with the errors measured on all
 * candidates and re-matches the rows that fail (match.cosine_topk). */
int pfr_topk_rescore_cert(const float* q, const float* g, const float* g_scale, int rows, int D, const int* cand, const float* cand_scores,
                          int KC, int K, float* out_scores, int* out_idx, float* cert, pfr_stream_t stream);
/* out[p] = (cos(emb[idx_a[p]], emb[idx_b[p]]) + 1) / 2, norms clamped at eps (F.cosine_similarity) */
int pfr_pair_similarity(const float* emb, int D, const long* idx_a, const long* idx_b, int P, float eps, float* out,
                        pfr_stream_t stream);

/* sort / scan part of the verification metrics (engine/controller.py:112-183; torchmetrics ROC / AUROC / AveragePrecision /
 * StatScores over the pair scores): scores fp32 [P], labels int32 [P] (0 impostor, != 0 genuine) -> sorted_scores [P] descending
 * (ties: lower pair index first), cum_tp [P] = genuine pairs among the first i+1, run_end [P] = 1 where a run of equal scores ends
 * (the distinct-threshold operating points).  workspace: pfr_pair_curve_ws_bytes(P). */
long pfr_pair_curve_ws_bytes(int P);
int pfr_pair_curve(const float* scores, const int* labels, int P, void* workspace, float* sorted_scores, int* cum_tp,
                   unsigned char* run_end, pfr_stream_t stream);

/* ---- all-pairs verification: genuine / impostor score histograms of EVERY pair, from the match GEMM with a histogram epilogue (the
 * score matrix is never written).  a [Na][D], b [Nb][D]: rows of `dtype` in the layouts of the match — PFR_F32 / PFR_BF16 rows with the
 * D multiples of pfr_match_scores_filter (128-byte k-steps: D % 32 == 0 / D % 64 == 0); PFR_I8 rows of pfr_quantize_rows_i8 with their
 * scales a_scale [Na], b_scale [Nb] (D = Dp, Dp % 128 == 0, Dp <= 1040 so that the int32 -> float conversion is exact); the scales are
 * NULL for the other dtypes.  a_cls [Na], b_cls [Nb]: int32 class of every row.  b == NULL: symmetric mode, every unordered pair i < j
 * of a is counted exactly once (b_scale, b_cls, Nb are ignored).
 *   Score s of (a row i, b row j): the fp32 accumulator (PFR_F32, PFR_BF16), or ((float) acc * a_scale[i]) * b_scale[j] (PFR_I8; the
 *     operations and the order of pfr_match_scores_i8).
 *   Bin rule (fp32, each operation rounded on its own, no fma):  x = (s - lo) * inv_w;  t = floorf(x);
 *     bin = (int) fminf(fmaxf(t, 0), bins - 1);  a NaN score goes to slot `bins`.  Scores outside the range therefore saturate into
 *     the first or the last bin.  1 <= bins <= 8192; inv_w > 0.
 *   kind = (a_cls[i] == b_cls[j]) ? 1 : 0;   hist[kind][bin] += 1   with hist u64 [2][bins + 1].
 * The call ADDS to hist (the caller zeroes it; chunked or sharded callers accumulate into one table).  Na == 0, Nb == 0 and a symmetric
 * Na == 1 add nothing and return 0.  Workgroup-private counters are 32-bit and are flushed after at most 2^16 tiles of 2^14 pairs. */
int pfr_pair_hist(const void* a, const float* a_scale, const int* a_cls, int Na, const void* b, const float* b_scale, const int* b_cls,
                  int Nb, int dtype, int D, float lo, float inv_w, int bins, unsigned long long* hist, pfr_stream_t stream);

/* pfr_pair_tile_coords (host only, no device needed): the tile queue of csrc/pfr_tilewalk.h, which pfr_rank_count, pfr_pairs_above and
 *   pfr_class_extremes walk (pfr_pair_hist, pfr_card_max_scores, pfr_neighbor_count and pfr_dbscan_link walk the same order with
 *   private copies of the arithmetic, which this entry does not run).  The Na x Nb score matrix is cut into 128 x 128 tiles and those
 *   into super-tiles of 16 x 16 tiles; slot t of the queue is tile t % 256 (row-major) of super-tile t / 256 (row-major; sym != 0,
 *   Na == Nb: the super-tiles of the upper triangle only).  For the slots t0 .. t0 + n - 1 coords [n][2] int32 receives the tile row
 *   and column, or -1, -1 for a slot that holds no tile (past the last tile row / column, or below the diagonal in symmetric mode).
 *   Every tile (symmetric: every tile with column >= row) is in exactly one slot.  The queue has 256 * (super-tile count) slots; slots
 *   outside it, Na or Nb < 1 and a symmetric Na != Nb return PFR_ERR_ARG. */
int pfr_pair_tile_coords(long t0, int n, int Na, int Nb, int sym, int* coords);

/* ---- exact retrieval ranks (mAP / CMC / mINP): the match GEMM with a RANK-COUNTING epilogue.  The rank of a positive is the number of
 * items that precede it, so it is counted where the MFMA leaves the scores; nothing Na x Nb is written and nothing is sorted.
 *   Scores.  a [Na][D], b [Nb][D], a_scale, b_scale, dtype, D: the operands, layouts and D multiples of pfr_pair_hist, and its score
 *     s(i, j): the fp32 accumulator (PFR_F32, PFR_BF16), or ((float) acc * a_scale[i]) * b_scale[j] (PFR_I8).  b == NULL means b = a
 *     (b_scale and Nb are then ignored; b_id is still the ids of those rows).
 *   Order.  Every b row carries a tie-break key b_id[j] (int32; a wrapper passes the caller's original index).  Item (s, id) PRECEDES
 *     threshold (t, tid) iff  s > t || (s == t && id < tid)  — the order of a stable descending argsort over the original indices.  The
 *     comparisons are IEEE: a NaN score precedes nothing and nothing precedes a NaN threshold.
 *   Thresholds and counts.  Per row i the thresholds thr_val[i][k] (fp32), thr_id[i][k] (int32) for k < thr_cnt[i] (int32 [Na], values
 *     outside [0, ld] are clamped), row stride ld, in any order:
 *       cnt[i][k] += #{ j in [0, Nb) : b_id[j] != excl[i] and (s(i, j), b_id[j]) precedes (thr_val[i][k], thr_id[i][k]) }
 *     excl int32 [Na], or NULL for no exclusion (a symmetric wrapper passes the query's own id: a query never ranks itself).
 *     cnt uint32 [Na][ld]; slots k >= thr_cnt[i] are not touched.  The call ADDS (chunked and sharded callers accumulate into one table;
 *     the caller zeroes it).  Integer adds only: two calls on the same inputs give the same bits.  Na == 0, Nb == 0 or ld == 0 adds
 *     nothing and returns 0.
 *   A launch takes at most pfr_rank_count_max_thr() thresholds per row (host-only query; 64: the thresholds and their 32-bit counters
 *     of a 128-row tile live in LDS, 128 x ld x 12 bytes next to 35 840 bytes of operands — 134 144 of the CU's 163 840 bytes at 64); a
 *     caller with longer lists slices them into several launches.  A larger ld returns PFR_ERR_ARG and launches nothing; so do null or
 *     host pointers, a bad dtype or D, and int8 rows without their scales.
 *
 * pfr_pair_scores_gather: out[i][k] = s(i, col[i][k]) for every col[i][k] in [0, Nb) (col int32 [Na][ld], out fp32 [Na][ld], any ld >= 0;
 *   other entries are padding: nothing is read through them and their out element is not touched).  This is where thresholds come from:
 *   the threshold of a positive (i, p) must be the very fp32 number the count launch computes for (i, p), or the positive could count
 *   itself.  THE TWO ENTRY POINTS AGREE BIT FOR BIT on the same operand bits: both run the same tile code — the same staging, 128-byte
 *   k-steps and MFMA sequence — and the same score expression; the gather multiplies the 128 rows of a row tile with the 128 gathered b
 *   rows of one k and keeps the diagonal, and an accumulator element depends on its two operand rows and the k order only, not on its
 *   place in a tile.  Same argument errors as pfr_rank_count. */
int pfr_rank_count_max_thr(void);
int pfr_rank_count(const void* a, const float* a_scale, int Na, const void* b, const float* b_scale, const int* b_id, int Nb, int dtype,
                   int D, const int* excl, const float* thr_val, const int* thr_id, const int* thr_cnt, int ld, unsigned int* cnt,
                   pfr_stream_t stream);
int pfr_pair_scores_gather(const void* a, const float* a_scale, int Na, const void* b, const float* b_scale, int Nb, int dtype, int D,
                           const int* col, int ld, float* out, pfr_stream_t stream);

/* ---- threshold clustering: range search and single-linkage components from the match GEMM (csrc/pfr_cluster.hip).  Nothing Na x Nb is
 * written: every score is compared with the threshold where the MFMA leaves it; what qualifies is appended to an edge list, united in a
 * parent array, or both.
 *   Scores.  a [Na][D], b [Nb][D], a_scale, b_scale, dtype, D: the operands, layouts and D multiples of pfr_pair_hist.  s(i, j) is the score
 *     of pfr_pair_hist / pfr_pair_scores_gather, produced by the tile code pfr_pair_scores_gather runs (csrc/pfr_pairtile.h: the same
 *     staging, 128-byte k-steps, MFMA sequence and score expression): the two AGREE BIT FOR BIT on the same operand bits.  b == NULL:
 *     symmetric mode, every unordered pair i < j of a is visited once, the diagonal never (b_scale, Nb and b_off are ignored).
 *   Rule.  A pair qualifies iff  s(i, j) >= thr  as an IEEE comparison: a NaN score never qualifies, thr = -inf takes every non-NaN pair,
 *     thr = +inf only +inf scores.  Node ids: u = a_off + i, v = b_off + j (symmetric: v = a_off + j) — a caller clusters a set too large
 *     for one launch block by block.
 *   Edge output (edge_i != NULL; edge_j and count are then required, edge_s is optional).  *count (u64, device) is INCREASED by the number
 *     of qualifying pairs of this call: the call adds, the caller zeroes it.  The pair that draws position p < cap is written as
 *     edge_i[p] = u, edge_j[p] = v, edge_s[p] = s; pairs that draw p >= cap are counted and not written, and nothing is written at or
 *     beyond cap: *count > cap after the call means "truncated, run again with cap >= *count".  Positions are reserved per wave and tile
 *     (the lanes' qualifying masks, their population counts, a wave scan, ONE agent-scope integer add by one lane); a wave whose 64 x 64
 *     part of a tile holds no qualifying score pays one wave vote.  The ORDER of the edges is unspecified; the SET is deterministic.
 *   Union output (parent != NULL; status is then required).  parent int32 [n_nodes] with 0 <= parent[x] <= x on entry (0, 1, 2, ... is
 *     the empty forest; the output of an earlier call is valid too: calls accumulate).  For every qualifying pair with both ids in
 *     [0, n_nodes) the two trees are united, lock-free: every access to parent is an agent-scope relaxed atomic load or compare-exchange
 *     (a plain store is not seen across XCDs).  A union finds both roots with path halving, hooks the LARGER root under the SMALLER with a
 *     compare-exchange and, when that fails, goes on from the value read back.  parent[x] <= x therefore holds at every instant and every
 *     walk strictly descends.
 *     NO UNBOUNDED LOOP: a union spends at most  6 * n_nodes + 64  loop iterations (find steps and hook retries together: both walks
 *     only descend and every failed hook descends too, so a correct forest needs fewer than 6 n_nodes — csrc/pfr_cluster.hip).  A union that reaches the cap, or reads a parent outside [0, x], stores a
 *     non-zero value to *status (int32, device; the caller zeroes it) and gives up on that pair: a bug or a corrupt parent array ends in a
 *     flag and a wrong answer, never in a hang or an access outside parent.
 *   Either output may be absent; both absent is PFR_ERR_ARG.  So are null or host pointers among the required arguments, a bad dtype or
 *     D, int8 rows without their scales, cap < 0, n_nodes < 0, negative offsets, and offsets that pass 2^31 - 1 together with Na / Nb; nothing
 *     is launched or written then.  Na == 0, Nb == 0 and a symmetric Na == 1 do nothing and return 0.
 *
 * pfr_cc_union: the same union over an explicit edge list edge_i / edge_j int32 [E] (from pfr_pairs_above, from top-K lists, from another
 *   rank).  Self-loops and edges with an id outside [0, n_nodes) are ignored (-1 is padding).  E == 0 does nothing.
 * pfr_cc_flatten: labels[x] = the root of x = the smallest node id of its component (int32 [n_nodes]).  The kernel only reads parent
 *   (agent-scope loads, walks bounded by n_nodes) and writes labels with agent-scope stores, so labels MAY ALIAS parent: a walker that
 *   meets a flattened entry reads either the old parent or the root, both ancestors.  It is a launch of its own: the kernel boundary is
 *   what makes every hook of the earlier launches visible.  The labels are canonical: two runs give the same bits whatever order the
 *   unions took.
 * NOT COVERED.  A threshold so low that the graph is near complete makes the union epilogue do ~N^2 / 2 finds: correct, slow, and not
 *   measured.  Single linkage only (connected components of the threshold graph); DBSCAN is the next section; no average linkage or
 *   Chinese whispers. */
int pfr_pairs_above(const void* a, const float* a_scale, int Na, int a_off, const void* b, const float* b_scale, int Nb, int b_off,
                    int dtype, int D, float thr, int* edge_i, int* edge_j, float* edge_s, long cap, unsigned long long* count,
                    int* parent, int n_nodes, int* status, pfr_stream_t stream);
int pfr_cc_union(int* parent, int n_nodes, const int* edge_i, const int* edge_j, long E, int* status, pfr_stream_t stream);
int pfr_cc_flatten(int* parent, int n_nodes, int* labels, pfr_stream_t stream);

/* ---- DBSCAN identity clustering from the match GEMM (csrc/pfr_dbscan.hip): two passes of the score GEMM of pfr_pairs_above — a degree
 * epilogue and a link epilogue — and a label pass.  Nothing N x N and no edge list is written.
 *   Scores, dtypes, operand preparation, the schedule and the qualifying rule are EXACTLY those of pfr_pairs_above (rc_tile_gemm / rc_score
 *     of csrc/pfr_pairtile.h: the bits of pfr_pair_scores_gather;  s >= thr  as an IEEE comparison, so a NaN score never qualifies).
 *     b == NULL: symmetric mode, every unordered pair i < j of a once; otherwise every pair of the two sets (the caller passes DISJOINT
 *     blocks of one node set).  Node ids: u = a_off + i, v = b_off + j (symmetric: v = a_off + j), all below n_nodes.
 *   Definition, over the unordered pairs i < j of ONE node set:
 *     deg[x]  = the number of OTHER nodes whose score with x qualifies.
 *     x is CORE iff deg[x] >= min_neighbors;  min_neighbors = min_samples - 1: the point itself counts towards min_samples (scikit-learn).
 *     CLUSTERS are the connected components of the core nodes over the qualifying core-core pairs; a cluster's label is its SMALLEST
 *       CORE INDEX.
 *     A non-core node with at least one qualifying core neighbour is a BORDER node: it takes the cluster of the core neighbour with the
 *       HIGHEST score, ties go to the SMALLEST index; -0.0 is canonicalised to +0.0 (s + 0.0f) before the comparison.  (This rule is
 *       this library's: scikit-learn gives a border node to whichever cluster reaches it first in its visiting order.)
 *     Every other node is NOISE: label -1.
 *     The result does not depend on scheduling, chunking or the number of calls: two runs give the same labels.
 * pfr_neighbor_count: for every visited qualifying pair (u, v), deg[u] += 1 and deg[v] += 1 (int32 [n_nodes], agent-scope relaxed atomic
 *   adds; deg is ACCUMULATED, the caller zeroes it, block launches add up).  The adds are reduced inside the wave first: a column's count
 *   is the population count of the lane's mask bits plus the same from the lane 32 away, a row's count is a wave vote over the 32 lanes
 *   that share the row; one add per touched row or column per wave and tile.
 * pfr_dbscan_link: deg is the finished output of pfr_neighbor_count (an earlier launch; read with plain loads).  parent int32 [n_nodes] as
 *   for pfr_pairs_above (0, 1, 2, ... on entry, calls accumulate), best u64 [n_nodes] zeroed by the caller, status int32 zeroed by the
 *   caller.  For every visited qualifying pair: both core -> the union of pfr_pairs_above (same loop cap of 6 * n_nodes + 64 iterations,
 *   same *status != 0 when it is reached or a parent outside [0, x] is read: never a hang, never a stray access); exactly one core c, the
 *   other node x -> an agent-scope atomic maximum on best[x] with the key
 *       (ord(s) << 32) | (0xffffffff - c),   ord(s) = bits(s + 0.0f) with all bits flipped when negative, the sign bit flipped otherwise
 *   (an order-preserving map of the floats to uint32), so that the maximum is "highest score, then smallest index"; best[x] == 0 means "no
 *   core neighbour": every real key is > 0.  Neither core -> nothing.
 * pfr_dbscan_labels: one thread per node.  Core -> the root of its tree (the read-only walk of pfr_cc_flatten, at most n_nodes steps,
 *   every parent range-checked); border -> the root of the core decoded from best (a key that decodes outside [0, n_nodes) is noise, never
 *   an index); noise -> -1.  labels int32 [n_nodes] must not alias the inputs.  A launch of its own, after every pfr_dbscan_link launch.
 * Errors (PFR_ERR_ARG, nothing launched or written): those of pfr_pairs_above — null or host pointers, a bad dtype or D, int8 rows
 *   without their scales, negative sizes or offsets — and  a_off + Na > n_nodes,  b_off + Nb > n_nodes  (no node is skipped silently),
 *   min_neighbors < 0.  Na == 0, Nb == 0, a symmetric Na == 1 (and n_nodes == 0 for the label pass) do nothing and return 0.
 * NOT COVERED.  Two-set (gallery against query) DBSCAN, average linkage, HDBSCAN / OPTICS, Chinese whispers; a threshold so low that the
 *   graph is near complete (correct, slow, not measured: as pfr_pairs_above). */
int pfr_neighbor_count(const void* a, const float* a_scale, int Na, int a_off, const void* b, const float* b_scale, int Nb, int b_off,
                       int dtype, int D, float thr, int* deg, int n_nodes, pfr_stream_t stream);
int pfr_dbscan_link(const void* a, const float* a_scale, int Na, int a_off, const void* b, const float* b_scale, int Nb, int b_off,
                    int dtype, int D, float thr, const int* deg, int min_neighbors, int* parent, unsigned long long* best, int n_nodes,
                    int* status, pfr_stream_t stream);
int pfr_dbscan_labels(const int* parent, const int* deg, const unsigned long long* best, int min_neighbors, int n_nodes, int* labels,
                      pfr_stream_t stream);

/* ---- open-set identification from the match GEMM (csrc/pfr_extremes.hip): per node the BEST MATE (highest same-class score), the BEST
 * IMPOSTOR (highest other-class score) and the WEAKEST MATE (lowest same-class score), each with its partner's index.  These are the
 * two numbers per probe that FNIR@FPIR / DIR@FAR needs, and what label cleaning and hard-pair mining read.  Nothing N x N is written.
 *   Operands, scores, schedule.  EXACTLY those of pfr_pairs_above / pfr_neighbor_count: rc_tile_gemm / rc_score of csrc/pfr_pairtile.h, so
 *     a score has the bits of pfr_pair_scores_gather; dtypes fp32, bf16 and int8 with row scales, the same D rules; persistent workgroups
 *     walk 128 x 128 tiles in 16 x 16 super-tiles, upper triangle only in symmetric mode.  b == NULL: symmetric mode, every unordered
 *     pair i < j of a is visited once and the diagonal never — an item is never its own mate (cls_b, b_scale, Nb, b_off and both_sides are
 *     ignored).  Otherwise every pair of the two sets is visited.
 *   Node ids.  u = a_off + i, v = b_off + j (symmetric: v = a_off + j).
 *   Classes.  cls_a int32 [Na], cls_b int32 [Nb]: the class of each row.  The pair (i, j) is a MATE pair iff cls_a[i] == cls_b[j] and
 *     cls_a[i] >= 0; every other pair is an IMPOSTOR pair.  A NEGATIVE class means "unlabelled / distractor": such a row has no mates and
 *     is an impostor to everyone, other distractors (of the same negative value too) included.
 *   Updates.  A pair whose score is NaN updates nothing (the gate is s == s).  Every other visited pair updates node u with partner v; in
 *     symmetric mode, or when both_sides != 0, it also updates node v with partner u.  With both_sides != 0 the caller passes DISJOINT
 *     blocks of one node set (as for pfr_dbscan_link: a set too large for one launch, block by block).  both_sides == 0 is the
 *     probe-against-gallery form: only the a side has outputs, v is merely the stored partner index.
 *   Keys.  best_pos, best_neg, worst_pos: u64 [n_nodes], ZEROED BY THE CALLER; calls accumulate, so block launches combine.  Every update
 *     is an agent-scope relaxed atomic maximum with the key
 *         best_pos[x], best_neg[x]:  ( ord(s) << 32) | (0xffffffff - partner)     — the maximum is the HIGHEST score, then the SMALLEST partner
 *         worst_pos[x]:              (~ord(s) << 32) | (0xffffffff - partner)     — the maximum is the LOWEST score, then the SMALLEST partner
 *     ord(s) = bits(s + 0.0f) with all bits flipped when negative, the sign bit flipped otherwise (the order-preserving uint32 of the
 *     DBSCAN border key: -0.0 is canonicalised to +0.0, csrc/pfr_scorekey.h); ~ is the 32-bit complement.  A mate pair updates best_pos
 *     and worst_pos, an impostor pair best_neg.  Key 0 means "no such pair": every real key is > 0 because partner < 2^31.  worst_pos
 *     may be NULL: it is then not computed; best_pos and best_neg are required.  The result depends on neither scheduling, chunking nor
 *     the number of calls: two runs give the same bits.
 *   Cost.  The atomics are reduced first.  A FILTER: per tile every row and column reads its node's current best_neg key once (agent-scope
 *     relaxed load; stale is safe, keys only grow) and an impostor score below it is dropped; one wave vote ends a wave in which nothing
 *     is left.  A WAVE REDUCTION of what is left: at most one atomic maximum per touched row or column, per kind, per wave and tile.
 *     Mate pairs are not filtered: the cost grows with the share of mate pairs (a set of few huge classes is correct and slow).
 * pfr_extremes_decode: one thread per key, keys u64 [n] -> score fp32 [n], index int32 [n].  kind 0: a max-key (best_pos, best_neg);
 *   kind 1: a min-key (worst_pos: the ~ is undone).  A non-zero key gives score = the float whose ord is stored, index = the partner;
 *   key 0 gives index = -1 and score = -inf (kind 0) or +inf (kind 1).  A key that decodes to an index >= 2^31 is treated as key 0 and is
 *   never used as an index.
 * Errors (PFR_ERR_ARG, nothing launched or written): those of pfr_neighbor_count — null or host pointers among the required arguments, a
 *   bad dtype or D, int8 rows without their scales, negative sizes or offsets, a_off + Na > n_nodes, b_off + Nb > n_nodes when the b side
 *   is written (symmetric mode, both_sides != 0), offsets that pass 2^31 - 1 together with Na / Nb — plus a null cls_a, a null cls_b in
 *   two-set mode, and for the decoding n < 0 and a kind outside {0, 1}.  Na == 0, Nb == 0, a symmetric Na == 1 and n == 0 do nothing
 *   and return 0.
 * Metrics on top (host arithmetic, engine.metrics.OpenSetStats of the Python package; every probe searched against all the others,
 *   leave-one-out).  Rank order is (score descending, index ascending).  MATED probes M = {x : best_pos index >= 0}; x is a HIT iff its
 *   best mate ranks before its best impostor, or it has no impostor.  rank1 = hits / |M|.  NON-MATED searches: every probe with an
 *   impostor, searched against the gallery without its own class — its top score is its best_neg score; n = their number;
 *   FPIR(t) = #{best_neg score >= t} / n;  t(f) = the smallest fp32 t with #{best_neg score >= t} <= floor(f n), i.e. nextafter above the
 *   (floor(f n) + 1)-th largest impostor score, -inf when floor(f n) >= n;  DIR@FPIR=f = #{x in M : hit and best_pos score >= t(f)} / |M|,
 *   FNIR = 1 - DIR.
 * NOT COVERED.  More than one extreme per row (the top-K match lists, match.cosine_topk, keep K of them); a per-class second-best. */
int pfr_class_extremes(const void* a, const float* a_scale, int Na, int a_off, const void* b, const float* b_scale, int Nb, int b_off,
                       int dtype, int D, const int* cls_a, const int* cls_b, int both_sides, unsigned long long* best_pos,
                       unsigned long long* best_neg, unsigned long long* worst_pos, int n_nodes, pfr_stream_t stream);
int pfr_extremes_decode(const unsigned long long* keys, int n, int kind, float* score, int* index, pfr_stream_t stream);

/* ---- k-reciprocal re-ranking of match lists (Zhong et al., "Re-ranking Person Re-identification with k-reciprocal Encoding", CVPR 2017)
 * on SPARSE rows: nothing N x N is built.  The set is N items with unit-norm fp32 rows emb32 [N][D].
 * Inputs
 *   nbr [N][K1] int32, K1 = k1 + 1: nbr[i][0] = i, then the k1 nearest OTHER items by descending cosine, padded with -1 when N - 1 < k1.
 *     Any entry outside [0, N) is padding and is skipped, wherever it stands; the kernels never use it as an address.
 *   cand [R][kc] int32 with cand_cos [R][kc] fp32: the candidates to be re-ranked for the R output rows rows [R], sorted by descending
 *     cosine, padded with -1 / -inf; kc <= 512 (the limit of the running top-K lists that produce them).
 * Definitions
 *   kh = round(k1 / 2) with halves to even, as Python's round() in the published code (k1 = 5 -> 2, k1 = 3 -> 2, k1 = 1 -> 0).
 *   L_k(i) = the first k + 1 valid entries of nbr[i].        R(i, k) = { j in L_k(i) : i in L_k(j) }.
 * Steps
 *   1. Expansion.  R*(i) = R(i, k1)  ∪  ⋃ { R(j, kh) : j in R(i, k1) and 3 |R(j, kh) ∩ R(i, k1)| > 2 |R(j, kh)| }; the intersection is
 *      taken with the UNEXPANDED R(i, k1); duplicates are removed.  Integer logic: exact.  Row capacity E = (k1 + 1) + (k1 + 1)(kh + 1).
 *   2. Weights.  For j in R*(i): d(i, j) = 2 - 2 <emb32[i], emb32[j]> (the squared Euclidean distance of unit rows, computed in fp32 from
 *      the rows, because j need not be in nbr[i]);  V[i][j] = exp(-d(i, j)) / Σ_j' exp(-d(i, j')).  Rows are stored padded (-1 / 0),
 *      sorted by ascending index, with a count.
 *      DEVIATION from the published code: that code first divides the distance matrix by its per-column maximum, which needs the N x N
 *      matrix; this normalisation is dropped.
 *   3. Local query expansion.  V'[i] = (1 / k2') Σ_{n in the first k2' valid entries of nbr[i]} V[n], k2' = min(k2, valid entries); self is
 *      included, as in the published code.  Capacity E2 = k2 E.  k2 = 1 is the identity (bit for bit).
 *   4. Scores.  For an output row i = rows[r] and each valid c = cand[r][t]:  m = Σ_j min(V'[i][j], V'[c][j]) over the common j;
 *      dJ = 1 - m / (2 - m) (exact Jaccard: both rows sum to 1);  final = (1 - lambda) dJ + lambda (2 - 2 cand_cos[r][t]).
 *      Output: the k smallest as dist [R][k] fp32 ascending with idx [R][k] int32 (= cand[r][t]); ties -> lower position t; padding +inf / -1.
 *      A row index rows[r] outside [0, N) gives an all-padding output row.
 * RESTRICTED CANDIDATE LISTS: re-ranking kc candidates equals re-ranking everything only when the list covers every other item — an item
 *   outside the list with a non-zero overlap m could otherwise enter the top k.
 * Determinism: every reduction runs in a fixed order, there are no floating-point atomics: two calls on the same inputs give the same bits.
 * One workgroup per row, lists and sets in LDS sized from E, E2 and kc; (k1, k2) whose rows do not fit the 160 KiB return
 * PFR_ERR_UNSUPPORTED.  Argument errors (null pointers, k1 < 1, k1 + 1 > 512, k2 < 1, kc > 512, k > kc, rows shorter than the capacity) return
 * PFR_ERR_ARG and launch nothing. */
/* host only, no device needed: E and E2 of (k1, k2) — the row lengths the caller's buffers need */
int pfr_rerank_row_capacity(int k1, int k2, int* E, int* E2);
/* steps 1 and 2: v_idx [N][cap] int32 (ascending, -1 padded), v_val [N][cap] fp32 (0 padded), v_cnt [N] int32; cap >= E */
int pfr_rerank_expand(const float* emb32, int N, int D, const int* nbr, int k1, int* v_idx, float* v_val, int* v_cnt, int cap,
                      pfr_stream_t stream);
/* step 3: the rows of pfr_rerank_expand (cap >= E) -> q_idx / q_val [N][cap2], q_cnt [N] in the same layout; cap2 >= E2 */
int pfr_rerank_average(const int* nbr, int N, int k1, int k2, const int* v_idx, const float* v_val, const int* v_cnt, int cap, int* q_idx,
                       float* q_val, int* q_cnt, int cap2, pfr_stream_t stream);
/* step 4 on the rows of pfr_rerank_average (row length cap2), including the per-row sort of the kc <= 512 values; 0 <= lambda <= 1 */
int pfr_rerank_score(const int* q_idx, const float* q_val, const int* q_cnt, int N, int cap2, const int* rows, int R, const int* cand,
                     const float* cand_cos, int kc, float lambda, int k, float* dist, int* idx, pfr_stream_t stream);

/* mean-strategy card matching (generate_tsv.py:71-78,91-125): centroid of the L2-normalised photo embeddings of each card;
 * seg [ncards+1] int64 row offsets; cent32 fp32 [ncards][D] (always written), cent (cent_dtype) optional copy */
int pfr_card_centroids(const float* emb, const long* seg, int ncards, int D, float eps, float* cent32, void* cent,
                       int cent_dtype, pfr_stream_t stream);

/* ---- max-strategy card matching (generate_tsv.py:81-88): the score of a card pair is the BEST photo pair.  The photo x photo score
 * GEMM of the match with a segmented-max epilogue over ragged card boundaries on both tile axes; nothing photo-matrix-sized is written.
 * Cards are photo rows q [Pq][D], g [Pg][D] (unit-normalised by the caller) with int64 row offsets seg [ncards+1]; an empty range is a
 * card without photos, allowed anywhere (consecutively and at both ends included).
 *
 * pfr_card_tiles (host only, no device needed): packs WHOLE cards greedily, in order, into tiles of at most 128 photo rows.
 *   tiles [cap][4] int32 records: first card, card count, first row (= seg[first card]), row count.  Returns the number of tiles; with
 *   tiles == NULL nothing is written (size query), a second call with cap >= that number fills the records (cap too small: PFR_ERR_ARG).
 *   A non-empty card opens a new tile when it does not fit the open one.  Empty cards belong to the tile of the NEXT non-empty card,
 *   trailing empty cards to the last tile; a table of only empty cards is one tile of 0 rows; ncards == 0 gives 0 tiles.  Every card
 *   belongs to exactly one tile, the rows of a tile are contiguous, and so every output element below is written by exactly one workgroup
 *   with a plain store.  A card above 128 photos returns PFR_ERR_UNSUPPORTED (the message names the card), decreasing offsets, a negative
 *   seg[0] or more than 2^31 - 1 rows PFR_ERR_ARG.
 *
 * pfr_card_max_scores: q, g rows of `dtype` PFR_F32 / PFR_BF16 with the D multiples of pfr_pair_hist (128-byte k-steps: D % 32 == 0 /
 *   D % 64 == 0).  q_seg / g_seg and the records q_tiles [n_qtiles][4] / g_tiles [n_gtiles][4] of pfr_card_tiles in DEVICE memory; Pq, Pg =
 *   photo rows, Qcards = query cards.  The records carry absolute card and row numbers: g_tiles may point into the middle of the gallery's
 *   table, at the first tile that holds a card of the window, with n_gtiles covering the last such tile (a chunked caller visits only the
 *   tiles of its chunk; records outside the window are skipped).
 *     out [Qcards][ld] fp32:  out[i][j - col0] = max over photos a of query card i, b of gallery card j of <q_a, g_b>
 *   for every query card i of the q tiles given and every gallery card j in [col0, col0 + n) that lies in a g tile given; each product is
 *   the fp32 accumulator of the MFMA; -inf when either card has no photos.  Elements outside the window are not touched (ld >= n).
 *   Tile rows past a tile's row count never enter a maximum.  Max is exactly associative and commutative and there are no floating-point
 *   atomics: the result is bit-identical between calls and independent of the tiling.  The kernel trusts the records to describe the
 *   offsets (it clamps every address derived from them, a mismatch gives wrong maxima, never an access outside q, g or out's rows).
 *
 * pfr_card_max_rescore: exact fp32 maxima of listed pairs.  q, g fp32 unit rows (D % 4 == 0, 16-byte aligned), cand [Q][kc] int32 gallery
 *   cards (kc <= 512; an entry outside [0, Gcards) is padding) -> out [Q][kc] fp32 = the max dot of (query card r, cand[r][t]), -inf for
 *   padding or an empty card.  One wave per pair; every dot product is accumulated from the rows in the fixed k order of the fp32 path of
 *   pfr_card_max_scores, so on fp32 rows the two give the same bits.
 * Argument errors (null or host pointers, bad dtype / D / window) return PFR_ERR_ARG and launch nothing. */
long pfr_card_tiles(const long* seg, int ncards, int* tiles, int cap);
int pfr_card_max_scores(const void* q, const long* q_seg, const int* q_tiles, int n_qtiles, int Pq, int Qcards, const void* g,
                        const long* g_seg, const int* g_tiles, int n_gtiles, int Pg, int dtype, int D, int col0, int n, float* out, int ld,
                        pfr_stream_t stream);
int pfr_card_max_rescore(const float* q, const long* q_seg, int Q, const float* g, const long* g_seg, int Gcards, int D, const int* cand,
                         int kc, float* out, pfr_stream_t stream);

/* head/body fusion of the inference ranking (generate_tsv.py:91-110), in place over `head_scores`.  head_scores,
 * body_scores: fp32 [rows][ld] centroid dot products of a query-card block against gallery cards col0..col0+n.
 * q_flags [rows], g_flags [all gallery cards] (indexed col0 + j): bit 0 = card has head vectors, bit 1 = has body
 * vectors, bits 2..7 = species `type` (1-based).  thresholds: HOST array of n_types floats (generate_tsv.py:107:
 * [0.9069641, 0.985643]).  Pairs the reference skips (type mismatch, both scores 0) become -inf. */
int pfr_card_fuse_scores(float* head_scores, const float* body_scores, int rows, int ld, int n, int col0,
                         const unsigned char* q_flags, const unsigned char* g_flags, const float* thresholds, int n_types,
                         pfr_stream_t stream);

/* ---- train-time augmentation on the device (configs/dog_fe/fe_dogs_config.py:17-26: RandomAdjustSharpness(0, 0.1),
 * RandomAutocontrast(0.3), RandomCrop((220, 220)), Resize((224, 224)), RandomRotation(5), ToTensor), bit-exact with the
 * Pillow arithmetic torchvision's PIL-image transforms run (oracle/augment_ref.py).
 * pfr_augment_params (HOST arrays in, HOST array out; no device work): flags int32 [N][4] = (apply sharpness, apply
 * autocontrast, crop top, crop left), angles float32 [N] degrees → records int32 [N][12] (the flags + Pillow's 16.16
 * fixed-point inverse rotation about the centre of the out_w x out_h image).  Upload `records` and pass it below.
 * pfr_augment_train: x uint8 [N][H][W][3] → y float32 [N][3][out_h][out_w] in [0, 1]; ws: pfr_augment_ws_bytes. */
int pfr_augment_params(const int* flags, const float* angles, int N, int out_w, int out_h, int* records);
long pfr_augment_ws_bytes(int N, int H, int W);
int pfr_augment_train(const unsigned char* x, int N, int H, int W, int crop_h, int crop_w, int out_h, int out_w,
                      const int* records, float* y, void* ws, pfr_stream_t stream);
/* geometry-first order of the body configs (configs/dog_fe/body_dog_fe.py:18-27): crop → resize → rotate to a uint8 image, then
 * sharpness (SMOOTH) and autocontrast on THAT image (their frame / lo-hi see the rotation's zero fill), then ToTensor.  Same
 * arguments and records as pfr_augment_train; ws: pfr_augment_geo_ws_bytes. */
long pfr_augment_geo_ws_bytes(int N, int out_h, int out_w);
int pfr_augment_train_geo(const unsigned char* x, int N, int H, int W, int crop_h, int crop_w, int out_h, int out_w,
                          const int* records, float* y, void* ws, pfr_stream_t stream);

/* ---- flip, ColorJitter, grayscale and erasing on the device (csrc/pfr_augment_color.hip), bit-exact with the Pillow arithmetic
 * torchvision's PIL-image transforms run (tools/color_augment_np.py is the restatement the tests pin against Pillow):
 * RandomHorizontalFlip = Image.transpose(FLIP_LEFT_RIGHT); ColorJitter = randperm(4) order of ImageEnhance.Brightness / Contrast /
 * Color (.enhance(f) = Image.blend(degenerate, img, f)) and adjust_hue (convert('HSV'), H += uint8(hue * 255), convert('RGB'));
 * RandomGrayscale = convert('L') on three channels; RandomErasing = tensor[..., i:i+h, j:j+w] = value after ToTensor.
 * pfr_augment_color_params (HOST arrays; no device work): per sample flip / gray flags int32 [N], order int32 [N][4] (a permutation of
 * the op ids 0 brightness, 1 contrast, 2 saturation, 3 hue, in the order they run), factors float32 [N][3] (brightness, contrast,
 * saturation), hue float32 [N] in [-0.5, 0.5]; ops_mask bit k = op k is on in this pipeline (an op that is off is dropped from the
 * order) → records int32 [N][12] = flip, gray, order[4] (-1 = none), the three factors' bit patterns, the hue shift byte, pad[2];
 * *mask_out = 1 (a sample flips) | 2 (jitter or grayscale runs) | 4 (Contrast runs: the per-image mean pass is needed).
 * pfr_augment_color: x uint8 [N][H][W][3] → out (same shape): flip → jitter → grayscale per the uploaded records; `mask` selects
 * the parts to honour (bits as above; 2 alone or 6 may run in place, out == x).  ws: pfr_augment_color_ws_bytes(N) (int64 L sums).
 * pfr_augment_erase_params (HOST): rects int32 [N][5] = (erase, i, j, h, w), value float32 [3] → records int32 [N][8] and the largest
 * rectangle's area; a rectangle outside the H x W image is refused.  pfr_augment_erase: y float32 [N][3][H][W] in place.
 * pfr_augment_train_geo_color: pfr_augment_train_geo with the pre-pass in the body order (flip → crop → resize → rotate →
 * ColorJitter → grayscale → sharpness → autocontrast → ToTensor); ws: pfr_augment_geo_color_ws_bytes. */
int pfr_augment_color_params(const int* flip, const int* gray, const int* order, const float* factors, const float* hue, int ops_mask,
                             int N, int* records, int* mask_out);
long pfr_augment_color_ws_bytes(int N);
int pfr_augment_color(const unsigned char* x, int N, int H, int W, const int* color_records, int mask, unsigned char* out, void* ws,
                      pfr_stream_t stream);
int pfr_augment_erase_params(const int* rects, const float* value, int N, int H, int W, int* records, int* max_area);
int pfr_augment_erase(float* y, int N, int H, int W, const int* erase_records, int max_area, pfr_stream_t stream);
long pfr_augment_geo_color_ws_bytes(int N, int H, int W, int out_h, int out_w, int color_mask);
int pfr_augment_train_geo_color(const unsigned char* x, int N, int H, int W, int crop_h, int crop_w, int out_h, int out_w,
                                const int* records, const int* color_records, int color_mask, float* y, void* ws, pfr_stream_t stream);

/* ---- fit stage: a ragged batch of uint8 HWC frames → one uniform uint8 canvas, bit-exact with Pillow (csrc/pfr_augment_fit.hip).
 * mode 0 RESIZE: Image.resize((canvas_w, canvas_h), BILINEAR) (simple / no-align configs, simple_fe_dog.py:17-31), with the
 * per-image sharpness / autocontrast pre-ops applied to the raw frame; mode 1 THUMBNAIL_PAD: Image.thumbnail((canvas_w, canvas_h),
 * BICUBIC, reducing_gap=2.0) + centred zero pad (`resize_with_padding` of the body configs, body_dog_fe.py:18-33).
 * pfr_augment_fit_params (HOST arrays; no device work): shapes int32 [N][2] = (H, W) → records int32 [N][32] and the 22-bit
 * fixed-point coefficient tables of both axes of every image in `coeffs` (capacity in ints: pfr_augment_fit_coeff_ints, -1 on
 * error).  Record: 0 H, 1 W, 2-3 target w / h (thumbnail size or the canvas), 4-5 reduce factors x / y, 6-9 reduce box, 10-13
 * fractional resize box (float32 bit patterns), 14-15 pad left / top, 16-17 x table offset in `coeffs` / taps, 18-19 y table
 * offset / taps, 20-21 sharpness / autocontrast flags (written 0: the caller sets them before the upload, RESIZE only), 22-23
 * size after the reduce, 24 mode, 25-26 horizontal / vertical pass needed.  A table is [out][2 + taps] = (first tap, count,
 * k...); a pass Pillow skips gets the identity table.  Frames with a side above 4096 or taller than 100:1 are refused.
 * pfr_augment_fit: data = the packed frames on the device, offsets = int64 [N] byte offset of each frame (device), records /
 * coeffs uploaded → out_u8 [N][canvas_h][canvas_w][3].  ws: pfr_augment_fit_ws_bytes(total bytes of data, N). */
long pfr_augment_fit_coeff_ints(int mode, const int* shapes, int N, int canvas_h, int canvas_w);
int pfr_augment_fit_params(int mode, const int* shapes, int N, int canvas_h, int canvas_w, int* records, int* coeffs,
                           long coeff_capacity);
long pfr_augment_fit_ws_bytes(long total_bytes, int N);
int pfr_augment_fit(const unsigned char* data, const long* offsets, const int* records, const int* coeffs, int N, int canvas_h,
                    int canvas_w, unsigned char* out_u8, void* ws, pfr_stream_t stream);

/* ---- landmark alignment: homography solve (host) and perspective warp (device) (csrc/pfr_align.hip) ----
 * The reference's preprocessor/align.py: fit a homography from 3 or 4 landmarks onto base_pts, warp the frame to dsize.
 * OpenCV is not available to this project, so bit-identity with a cv2 build cannot be tested and is NOT claimed.  The contract
 * below is ours.  It follows OpenCV's published scheme for warpPerspective(..., INTER_LINEAR, BORDER_CONSTANT 0): inverse map in
 * fp64, source coordinates quantised to 1/32 pixel, 15-bit integer weights.  It fixes every operation.  It is pinned two ways: a
 * numpy restatement (tests/align_oracle.py), which the device must equal bit for bit, and Pillow's Image.transform(PERSPECTIVE,
 * BILINEAR), an independent implementation, which must lie within a derived bound of the restatement (tests/test_align_host.py).
 *
 * pfr_align_solve (HOST arrays; no device work): pts fp64 [N][npts][2] = (x, y), base fp64 [npts][2] → minv fp64 [N][9], the
 * INVERSE map (output pixel → source pixel, inverted in fp64 by the adjugate; the warp never inverts anything), and valid [N].
 *   mode 0 `reference` (npts 3 or 4): with 3 points the centroid of the three is prepended to both point sets, each coordinate
 *     rounded half-to-even (np.round(np.mean(...)), align.py:8-9); then the exact homography through the 4 correspondences: an 8x8
 *     system in fp64 with partial pivoting, h33 = 1.  With exactly four correspondences the reference's RANSAC + refinement has
 *     nothing to choose or refine, which is why the exact solve is the restatement.
 *   mode 1 `similarity` (npts >= 2): the least-squares rotation + uniform scale + translation, the 2-D closed form with no
 *     reflection; last row 0 0 1.
 *   valid[n] = 0 with minv[n] all zeros when two landmarks are not more than min_distance apart (the reference's strict
 *   `assert all(i > self.min_distance ...)`), when the system is singular (a pivot below 1e-12 x the largest entry, or the solved
 *   map does not return the points to 1e-6 px; similarity: a degenerate spread or scale), or when any entry is non-finite.
 *   The call still returns 0: an invalid frame is data, not an error.
 *
 * pfr_align_warp: data / offsets = the ragged batch exactly as pfr_augment_fit takes it, shapes int32 [N][2] = (H, W) and minv
 * [N][9] on the device.  mask may be NULL; otherwise packed uint8 [H][W] planes, each starting on a 16-byte boundary, at
 * mask_offsets int64 [N] (device); a zero byte drops the pixel.  out_u8 [N][out_h][out_w][3].  For output pixel (x, y) of frame n
 * with m = minv[n], every step in IEEE double, in this order, with NO fused multiply-add:
 *   X0 = (m0*x + m1*y) + m2, Y0 = (m3*x + m4*y) + m5, W0 = (m6*x + m7*y) + m8;  s = W0 != 0 ? 32.0 / W0 : 0.0;
 *   fx = X0*s, fy = Y0*s; a non-finite fx or fy makes the pixel 0,0,0, and so does the all-zero matrix, pfr_align_solve's mark of
 *   a rejected frame (by the steps above alone it would sample source pixel (0, 0) everywhere); otherwise clamp to [-2^31, 2^31-1] and round to nearest,
 *   ties to even → integers X, Y;  ix = X >> 5 (arithmetic), ax = X & 31; the same for y.
 *   Taps (iy, ix), (iy, ix+1), (iy+1, ix), (iy+1, ix+1) with weights (32-ax)(32-ay)*32, ax(32-ay)*32, (32-ax)ay*32, ax*ay*32 (sum
 *   32768); a tap outside the frame, or whose mask byte is 0, contributes 0; channel = (sum w*p + 16384) >> 15.
 * No address is formed from a coordinate that has not passed the per-tap range test; offsets are 64-bit.  One thread per output
 * pixel, no LDS, no atomics: bit-reproducible.  gfx950 build: 22 VGPRs, no scratch.  N == 0 or an empty output returns 0 without a
 * launch; an output side above 4096 or a null required pointer is PFR_ERR_ARG. */
int pfr_align_solve(int mode, const double* pts, const double* base, int N, int npts, double min_distance, double* minv, int* valid);
int pfr_align_warp(const unsigned char* data, const long* offsets, const int* shapes, const double* minv, const unsigned char* mask,
                   const long* mask_offsets, int N, int out_h, int out_w, unsigned char* out_u8, pfr_stream_t stream);

/* Linear layer with a fused activation epilogue — the Swin MLP `FeedForward` (reference models/swin.py:40-52: Linear →
 * GELU → Linear) and its autograd.  x [M][K], w [N][K] (nn.Linear layout), y / y2 [M][N], all of `dtype`.
 *   act 2: y2 = x·wT + bias (pre-activation, kept for backward), y = gelu(y2)            (forward of the first Linear)
 *   act 3: y = (x·wT) * gelu'(y2)                         (data gradient of the second Linear joined with GELU backward) */
int pfr_gemm_act(const void* x, const void* w, void* y, int dtype, long M, int K, int N, const float* bias, int act,
                 void* y2, pfr_stream_t stream);
/* the same + per-m-tile column statistics of the stored y in stats_part [ceil(M / mtile)][2][N] (mtile = pfr_conv2d_mtile(M, N, K, K,
 * dtype, dtype, 0)): a bias gradient (column sum of y) without another pass over y (pfr_colsum_final_batch, mt > 0) */
int pfr_gemm_act_colstats(const void* x, const void* w, void* y, int dtype, long M, int K, int N, const float* bias, int act,
                          void* y2, float* stats_part, pfr_stream_t stream);
/* act 3 (y = (x wT) * gelu'(y2), no bias) + plain column SUMS of the stored y: sums_part [parts][N] fp32 with parts =
 * pfr_gemm_act_colsum_parts(M, K, N, dtype); every partial row holds the column sums over a disjoint set of rows (their total = the bias
 * gradient of the Linear layer in front: pfr_colsum_final_batch with mt = 0).  Provided by the streaming Linear kernel (csrc/pfr_slin.hip)
 * for its geometries only: parts == 0 -> pfr_gemm_act_colstats.  The answer depends on the "slin" knobs (pfr_tuning_epoch). */
int pfr_gemm_act_colsum_parts(long M, int K, int N, int dtype);
int pfr_gemm_act_colsums(const void* x, const void* w, void* y, int dtype, long M, int K, int N, void* y2, float* sums_part,
                         pfr_stream_t stream);

/* ---- depthwise K x K convolution and layer scale of the ConvNeXt block (csrc/pfr_dwconv.hip; torchvision convnext.py CNBlock)
 * NHWC, stride 1, padding K/2, groups = C.  Only K = 7 is built: any other K returns PFR_ERR_UNSUPPORTED; C must be a multiple of the
 * 16-byte chunk (4 fp32 / 8 bf16); host pointers are refused with an error code.  w: tap-major [K*K][C] in the compute dtype (engine:
 * pfr_nchw_to_nhwc of the [C][1][K][K] parameter); bias fp32 [C] or NULL; fp32 accumulation.  flip = 1 reads the taps mirrored: the same
 * call is the data gradient, dx = pfr_dwconv2d_fwd(dy, w, NULL, dx, ..., flip = 1). */
int pfr_dwconv2d_fwd(const void* x, const void* w, const float* bias, void* y, int dtype, int N, int H, int W, int C, int K,
                     int flip, pfr_stream_t stream);
/* dw[c][kh][kw] = sum_{n,h,w} dy[n,h,w,c] * x[n,h+kh-K/2,w+kw-K/2,c] written in the parameter's own [C][1][K][K] order, dbias[c] = sum dy
 * (dbias may be NULL), both fp32; accumulate = 1 adds to what dw / dbias hold.  part_ws: fp32 [pfr_dwconv2d_wgrad_parts(...)][K*K+1][C]
 * per-workgroup partial sums, merged by a second launch of the same call (0 parts: geometry not supported). */
int pfr_dwconv2d_wgrad_parts(int dtype, int N, int H, int W, int C, int K);
int pfr_dwconv2d_wgrad(const void* x, const void* dy, float* part_ws, float* dw, float* dbias, int dtype, int N, int H, int W, int C,
                       int K, int accumulate, pfr_stream_t stream);
/* y = residual + row_scale[n] * gamma[c] * u over [N][HW][C]: layer scale with per-sample ("row" mode) stochastic depth; gamma fp32 [C],
 * row_scale fp32 [N] (0 or 1/(1-p)) or NULL = all ones */
int pfr_layer_scale_fwd(const void* u, const float* gamma, const float* row_scale, const void* residual, void* y, int dtype, int N,
                        int HW, int C, pfr_stream_t stream);
/* du = row_scale * gamma * dz; dgamma[c] = sum row_scale * dz * u through dgamma_part (fp32 [pfr_layer_scale_bwd_parts(N, HW, C)][C]).
 * dgamma != NULL: merged here (accumulate = 1 adds to dgamma); NULL: the caller merges the partial rows (pfr_colsum_final_batch). */
int pfr_layer_scale_bwd_parts(int N, int HW, int C);
int pfr_layer_scale_bwd(const void* dz, const void* u, const float* gamma, const float* row_scale, void* du, float* dgamma_part,
                        float* dgamma, int dtype, int N, int HW, int C, int accumulate, pfr_stream_t stream);

/* ---- depthwise 3x3 convolution of the MobileNetV2 inverted-residual block (csrc/pfr_dwconv3.hip; torchvision mobilenetv2.py
 * InvertedResidual: Conv2d(hidden, hidden, 3, stride, 1, groups=hidden, bias=False) between BatchNorm + ReLU6 pairs)
 * NHWC, padding 1, stride 1 or 2 (any other stride returns PFR_ERR_UNSUPPORTED), no bias, OH = (H - 1) / stride + 1 (OW likewise); C must
 * be a multiple of the 16-byte chunk (4 fp32 / 8 bf16); fp32 accumulation; host pointers are refused with an error code and an argument
 * error never launches.  w: tap-major [9][C] in the compute dtype (engine: pfr_nchw_to_nhwc of the [C][1][3][3] parameter).
 *   pro_scale / pro_shift fp32 [C] or both NULL: the operand is a = min(max(scale[c]*x + shift[c], 0), pro_hi), computed in fp32 from the
 *   stored x (the producer's BatchNorm apply + ReLU6; pro_hi = 6) — pro_hi <= 0: no upper clamp.  Taps outside the image contribute 0:
 *   the padding is of the ACTIVATED tensor, not of x.
 *   stats_part or NULL: fp32 [ceil(N*OH*OW / rpp)][2][C] per-channel (mean, M2) of the row groups [t*rpp, (t+1)*rpp) of the stored
 *   (rounded) y, rpp = pfr_dwconv3_rows_per_part(...) — the input of pfr_bn_finalize(part, nparts, rpp, ...); deterministic, no atomics. */
long pfr_dwconv3_rows_per_part(int dtype, int N, int H, int W, int C, int stride);
int pfr_dwconv3_fwd(const void* x, const void* w, void* y, int dtype, int N, int H, int W, int C, int stride, const float* pro_scale,
                    const float* pro_shift, float pro_hi, float* stats_part, pfr_stream_t stream);
/* dx [N][H][W][C] from dy [N][OH][OW][C]: a gather per dx pixel over the taps whose parity meets an output pixel (no atomics, no
 * zero-fill pass; every dx element is written) */
int pfr_dwconv3_dgrad(const void* dy, const void* w, void* dx, int dtype, int N, int H, int W, int C, int stride, pfr_stream_t stream);
/* dw[c][kh][kw] = sum_{n,oh,ow} dy[n,oh,ow,c] * a[n, oh*stride - 1 + kh, ow*stride - 1 + kw, c] in the parameter's own [C][1][3][3]
 * order, fp32; a = the activated operand recomputed with the forward's prologue (so the forward need not store it); accumulate = 1 adds
 * to what dw holds.  part_ws: fp32 [pfr_dwconv3_wgrad_parts(...)][9][C] per-workgroup partial sums, merged by a second launch of the
 * same call (0 parts: geometry not supported). */
int pfr_dwconv3_wgrad_parts(int dtype, int N, int H, int W, int C, int stride);
int pfr_dwconv3_wgrad(const void* x, const void* dy, float* part_ws, float* dw, int dtype, int N, int H, int W, int C, int stride,
                      const float* pro_scale, const float* pro_shift, float pro_hi, int accumulate, pfr_stream_t stream);
/* ReLU6 forms of the BatchNorm apply / backward (csrc/pfr_elementwise.hip; nn.ReLU6 = hardtanh(., 0, 6) after nn.BatchNorm2d).  The
 * entry points above are unchanged; these carry the upper bound `hi` (hi <= 0: none) and check every pointer to be device memory.
 *   pfr_bn_act_clamp:         y = min(max(a*x + b, 0), hi)                  (hi <= 0: pfr_bn_act(relu = 1), bit for bit)
 *   pfr_bn_bwd_reduce_clamp:  g = dout * [0 < scale*x + shift < hi], both strict (torch's hardtanh_backward), recomputed from the
 *                             BatchNorm input x (mask_mode 2; hi <= 0: pfr_bn_bwd_reduce's mask_mode 2, bit for bit) or g = dout
 *                             (mask_mode 0: a BatchNorm without activation); partials of (Σg, Σg·x̂) in pfr_bn_bwd_reduce's layout
 *                             ([pfr_colreduce_blocks(C, dtype, rows)][2][C]) for pfr_bn_bwd_finalize
 *   pfr_bn_bwd_apply_clamp:   dx = coef0*g + coef1*x + coef2 with the same g (dx may alias dout) */
int pfr_bn_act_clamp(const void* x, const float* a, const float* b, void* y, float hi, int dtype, long rows, int C,
                     pfr_stream_t stream);
int pfr_bn_bwd_reduce_clamp(const void* dout, const void* x, const float* mean, const float* invstd, const float* scale,
                            const float* shift, float hi, int mask_mode, int dtype, long rows, int C, float* part,
                            pfr_stream_t stream);
int pfr_bn_bwd_apply_clamp(const void* dout, const void* x, const float* coef, const float* scale, const float* shift, float hi,
                           int mask_mode, void* dx, int dtype, long rows, int C, pfr_stream_t stream);

/* ---- depthwise K x K convolution of the EfficientNet MBConv block (csrc/pfr_dwconvk.hip; torchvision efficientnet.py MBConv:
 * Conv2dNormActivation(expanded, expanded, kernel_size=k, stride=s, groups=expanded, activation_layer=SiLU), i.e.
 * Conv2d(C, C, k, s, (k - 1) // 2, groups=C, bias=False) between BatchNorm + SiLU pairs)
 * The contract of pfr_dwconv3_* plus `int K` (3 or 5, padding K/2; any other K or a stride other than 1 | 2 returns
 * PFR_ERR_UNSUPPORTED) and `int pro_act`, the producer's BatchNorm apply + activation as a prologue computed in fp32 from the stored x:
 *   0  the operand is x itself (pro_scale / pro_shift are not read)
 *   1  min(max(scale[c]*x + shift[c], 0), pro_hi)  (pro_hi <= 0: no upper clamp) — at K = 3 bit for bit pfr_dwconv3_fwd
 *   2  silu(scale[c]*x + shift[c]), the sigmoid in fp32
 * The padding is of the ACTIVATED tensor.  w: tap-major [K*K][C] in the compute dtype.  stats_part or NULL: fp32
 * [ceil(N*OH*OW / rpp)][2][C] (mean, M2) partials of the stored, rounded y, rpp = pfr_dwconvk_rows_per_part(...), the input of
 * pfr_bn_finalize.  OH = (H - 1) / stride + 1.  Deterministic, no atomics; an argument error never launches. */
long pfr_dwconvk_rows_per_part(int dtype, int N, int H, int W, int C, int K, int stride);
int pfr_dwconvk_fwd(const void* x, const void* w, void* y, int dtype, int N, int H, int W, int C, int K, int stride, int pro_act,
                    const float* pro_scale, const float* pro_shift, float pro_hi, float* stats_part, pfr_stream_t stream);
/* dx [N][H][W][C] from dy [N][OH][OW][C]: a gather per dx pixel (no atomics, no zero-fill pass; every dx element is written) */
int pfr_dwconvk_dgrad(const void* dy, const void* w, void* dx, int dtype, int N, int H, int W, int C, int K, int stride,
                      pfr_stream_t stream);
/* dw in the parameter's own [C][1][K][K] order, fp32, from the activated operand recomputed with the forward's prologue; accumulate = 1
 * adds to what dw holds.  part_ws: fp32 [pfr_dwconvk_wgrad_parts(...)][K*K][C] (0 parts: geometry not supported). */
int pfr_dwconvk_wgrad_parts(int dtype, int N, int H, int W, int C, int K, int stride);
int pfr_dwconvk_wgrad(const void* x, const void* dy, float* part_ws, float* dw, int dtype, int N, int H, int W, int C, int K, int stride,
                      int pro_act, const float* pro_scale, const float* pro_shift, float pro_hi, int accumulate, pfr_stream_t stream);
/* SiLU forms of the BatchNorm apply / backward (csrc/pfr_elementwise.hip; torchvision efficientnet.py: activation_layer=nn.SiLU after
 * nn.BatchNorm2d), beside the _clamp forms and with their layouts:
 *   pfr_bn_act_silu:         y = silu(a*x + b) = u * sigmoid(u), sigmoid in fp32
 *   pfr_bn_bwd_reduce_silu:  g = dout * sigmoid(u) * (1 + u * (1 - sigmoid(u))), u = scale*x + shift recomputed from the BatchNorm input x
 *                            (no mask, no stored activation); partials of (Σg, Σg·x̂) for pfr_bn_bwd_finalize
 *   pfr_bn_bwd_apply_silu:   dx = coef0*g + coef1*x + coef2 with the same g (dx may alias dout) */
int pfr_bn_act_silu(const void* x, const float* a, const float* b, void* y, int dtype, long rows, int C, pfr_stream_t stream);
int pfr_bn_bwd_reduce_silu(const void* dout, const void* x, const float* mean, const float* invstd, const float* scale,
                           const float* shift, int dtype, long rows, int C, float* part, pfr_stream_t stream);
int pfr_bn_bwd_apply_silu(const void* dout, const void* x, const float* coef, const float* scale, const float* shift, void* dx, int dtype,
                          long rows, int C, pfr_stream_t stream);
/* PReLU forms of the BatchNorm apply / backward (csrc/pfr_prelu.hip; insightface arcface_torch iresnet.py: `self.prelu = nn.PReLU(planes)`
 * after `self.bn2`, i.e. F.prelu(F.batch_norm(x, ...), weight) and its autograd), beside the _clamp / _silu forms and with their
 * layouts and checks.  u = scale[c]*x + shift[c], slope [C] fp32 (the nn.PReLU weight as it stands):
 *   pfr_bn_act_prelu:         y = u > 0 ? u : slope[c]*u   (eval mode: the same kernel on the coefficients of pfr_bn_eval_coeff)
 *   pfr_bn_bwd_reduce_prelu:  g = dout * (u > 0 ? 1 : slope[c]), u recomputed from the BatchNorm input x (no mask, no stored activation).
 *                             part: fp32 [nb][2][C] rows (Σg, Σg·x̂) per row block — pfr_bn_bwd_finalize reads them as they stand — followed
 *                             by [nb][C] rows Σ dout*min(u, 0), the slope gradient (u == 0 contributes 0, as torch's prelu_backward):
 *                             3*nb*C floats, nb = pfr_colreduce_blocks(C, dtype, rows).  Deterministic, no atomics.
 *   pfr_prelu_slope_finalize: the SEPARATE finalize of the third rows (pfr_bn_bwd_finalize stays as it is for dgamma, dbeta and coef):
 *                             dslope[c] = Σ_b part[2*nparts*C + b*C + c] (+ dslope[c] if accumulate); `part`, `nparts` as given to
 *                             pfr_bn_bwd_reduce_prelu / pfr_bn_bwd_finalize
 *   pfr_bn_bwd_apply_prelu:   dx = coef0*g + coef1*x + coef2 with the same g (dx may alias dout) */
int pfr_bn_act_prelu(const void* x, const float* scale, const float* shift, const float* slope, void* y, int dtype, long rows, int C,
                     pfr_stream_t stream);
int pfr_bn_bwd_reduce_prelu(const void* dout, const void* x, const float* mean, const float* invstd, const float* scale,
                            const float* shift, const float* slope, int dtype, long rows, int C, float* part, pfr_stream_t stream);
int pfr_prelu_slope_finalize(const float* part, int nparts, int C, float* dslope, int accumulate, pfr_stream_t stream);
int pfr_bn_bwd_apply_prelu(const void* dout, const void* x, const float* coef, const float* scale, const float* shift,
                           const float* slope, void* dx, int dtype, long rows, int C, pfr_stream_t stream);

/* ---- squeeze-and-excitation of the MBConv block (csrc/pfr_se.hip; torchvision ops/misc.py SqueezeExcitation.forward:
 * `scale = scale_activation(fc2(activation(fc1(avgpool(input))))); return scale * input` with activation = SiLU, scale_activation =
 * Sigmoid).  Activations NHWC [N][HW][C] in `dtype`, C a multiple of the 16-byte chunk; the squeeze is pfr_avgpool_fwd (pooled [N][C] in
 * `dtype`).  w1 = fc1.weight fp32 [S][C], b1 = fc1.bias [S], w2 = fc2.weight fp32 [C][S], b2 = fc2.bias [C], read from the fp32 master
 * parameters as they stand; S is any positive integer.  pre / gate / dgate / dpooled are fp32.  Deterministic, no atomics.
 *   pfr_se_gate_fwd:          pre[n][s] = b1[s] + Σ_c w1[s][c] pooled[n][c];  gate[n][c] = sigmoid(b2[c] + Σ_s w2[c][s] silu(pre[n][s]))
 *   pfr_se_scale_fwd:         y = a * gate[n][c]
 *   pfr_se_scale_bwd_reduce:  dgate[n][c] = Σ_hw dy * a
 *   pfr_se_gate_bwd:          dpooled [N][C] and the gradients of fc1 / fc2 (sums over N in ascending order; accumulate = 1 adds to what
 *                             dw1 / db1 / dw2 / db2 hold); dpre_ws: fp32 [N][S] workspace
 *   pfr_se_bwd_apply:         da = dy * gate[n][c] + dpooled[n][c] / HW */
int pfr_se_gate_fwd(const void* pooled, const float* w1, const float* b1, const float* w2, const float* b2, float* pre, float* gate,
                    int dtype, int N, int C, int S, pfr_stream_t stream);
int pfr_se_scale_fwd(const void* a, const float* gate, void* y, int dtype, int N, int HW, int C, pfr_stream_t stream);
int pfr_se_scale_bwd_reduce(const void* dy, const void* a, float* dgate, int dtype, int N, int HW, int C, pfr_stream_t stream);
int pfr_se_gate_bwd(const float* dgate, const void* pooled, const float* pre, const float* gate, const float* w1, const float* w2,
                    float* dpre_ws, float* dpooled, float* dw1, float* db1, float* dw2, float* db2, int dtype, int N, int C, int S,
                    int accumulate, pfr_stream_t stream);
int pfr_se_bwd_apply(const void* dy, const float* gate, const float* dpooled, void* da, int dtype, int N, int HW, int C,
                     pfr_stream_t stream);
/* per-sample ("row" mode) stochastic depth on the project BatchNorm (torchvision efficientnet.py MBConv.forward:
 * `result = self.stochastic_depth(result); result += input`): y = residual + row_scale[n] * (a[c]*z + b[c]), row_scale fp32 [N] of 0 or
 * 1/(1-p); backward: pfr_row_scale (y = row_scale[n] * x) in front of the linear pfr_bn_bwd_* path */
int pfr_bn_residual_rows(const void* z, const float* a, const float* b, const void* residual, const float* row_scale, void* y, int dtype,
                         int N, int HW, int C, pfr_stream_t stream);
int pfr_row_scale(const void* x, const float* row_scale, void* y, int dtype, int N, int HW, int C, pfr_stream_t stream);

/* ---- fused multi-head self-attention over the whole token sequence (csrc/pfr_mha.hip; torchvision vision_transformer.py
 * EncoderBlock: `self.self_attention(x, x, x, need_weights=False)` between in_proj and out_proj) ----------------------------------
 * qkv [B][S][3*heads*head_dim] (q|k|v, each (head, d)): the row layout nn.MultiheadAttention's in_proj produces and pfr_window_attn_*
 * already uses.  out [B][S][heads*head_dim]; lse fp32 [B][heads][S] (log-sum-exp of the scaled scores, saved for the backward; may be
 * NULL in inference).  head_dim == 64 and 1 <= S <= 257, fp32 or bf16: pfr_mha_supported (host arithmetic only) is 1 when a kernel
 * takes the shape, and any other shape is an argument error of pfr_mha_fwd / pfr_mha_bwd, never a different computation.
 * The B*heads*S*S scores are never written to memory.  bf16: one workgroup per (batch, head), K / V (backward: Q, K, V, dout) rows
 * in LDS with zero-filled padding rows, MFMA products, fp32 softmax with a running maximum, P rounded to bf16.  Backward = the
 * recompute form (P = exp(s - lse), D = rowsum(dout * out)); dqkv [B][S][3*heads*head_dim] is OVERWRITTEN, complete per workgroup:
 * no atomics, bit-reproducible.  Rows at or beyond S are never stored. */
int pfr_mha_fwd(const void* qkv, void* out, float* lse, int dtype, int B, int S, int heads, int head_dim, float scale, pfr_stream_t stream);
int pfr_mha_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int dtype, int B, int S, int heads,
                int head_dim, float scale, pfr_stream_t stream);
int pfr_mha_supported(int dtype, int S, int heads, int head_dim);
/* token assembly of the Vision Transformer (activations in `dtype`, D a multiple of the 16-byte chunk; class_token [D] and pos [S][D]
 * are the fp32 master parameters, their gradients fp32 and OVERWRITTEN, sums over b in ascending order):
 *   pfr_vit_tokens_fwd:  tok[b][0] = class_token + pos[0];  tok[b][s] = patches[b][s-1] + pos[s]     (patches [B][S-1][D], tok [B][S][D])
 *   pfr_vit_tokens_bwd:  dpatches[b][s-1] = dtok[b][s];  dpos[s] = sum_b dtok[b][s];  dclass_token = sum_b dtok[b][0]
 *   pfr_vit_cls_fwd:     y[b] = x[b][0]                          (the class-token rows, [B][D], that encoder.ln and the head read)
 *   pfr_vit_cls_bwd:     dx[b][0] = dy[b], dx[b][s > 0] = 0 */
int pfr_vit_tokens_fwd(const void* patches, const float* class_token, const float* pos, void* tok, int dtype, int B, int S, int D,
                       pfr_stream_t stream);
int pfr_vit_tokens_bwd(const void* dtok, void* dpatches, float* dpos, float* dclass_token, int dtype, int B, int S, int D,
                       pfr_stream_t stream);
int pfr_vit_cls_fwd(const void* x, void* y, int dtype, int B, int S, int D, pfr_stream_t stream);
int pfr_vit_cls_bwd(const void* dy, void* dx, int dtype, int B, int S, int D, pfr_stream_t stream);

/* ---- gradient all-reduce over RCCL / xGMI (csrc/pfr_comm.hip) ---------------------------------------------
 * For hosts that bind this library directly; replaces DistributedDataParallel's bucket all-reduce (utils/__init__.py:114-119).
 * RCCL is resolved with dlopen at first use (no load-time dependency).  pfr_comm_unique_id: rank 0 fills a 128-byte id, the
 * host distributes it; pfr_comm_init: one communicator per process / GPU (current HIP device), NULL on error;
 * pfr_comm_allreduce: in place, `count` elements of dtype, mean over the ranks when average != 0, asynchronous and ORDERED on `stream`: the
 * collective itself runs on a high-priority stream the communicator owns (so that it does not share a hardware queue with the caller's compute
 * streams), tied to `stream` by an event on either side — work enqueued on `stream` before the call is complete before the collective reads
 * `buf`, work enqueued after it sees the reduced values. */
int pfr_comm_unique_id(void* id128);
void* pfr_comm_init(int rank, int world, const void* id128);
int pfr_comm_allreduce(void* comm, void* buf, size_t count, int dtype, int average, pfr_stream_t stream);
int pfr_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* PFR_HIP_H */
