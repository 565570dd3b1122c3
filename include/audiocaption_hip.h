/*
 * C ABI of libaudiocaption_hip.so - the MI355X (gfx950) kernels behind the audio-captioning hot path
 *     wav -> log-mel -> Cnn14 -> bi-GRU -> Transformer decoder (greedy / beam).
 *
 * The reference (wsntxxn/AudioCaption) is pure Python/PyTorch and has no FFI: its boundary is the
 * Python plugin protocol.  This library sits UNDER the Python classes of
 * audiocaption_amd/ that mirror that protocol; each entry point names the reference code it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked "host";
 *   - float = IEEE fp32; token ids are int32 on the device side, int64 in the seq output
 *     (the reference returns int64, base.py:122);
 *   - `stream` is a hipStream_t (pass the caller's current PyTorch stream); all work is stream-ordered,
 *     nothing synchronises, nothing allocates; outputs are caller-allocated;
 *   - return value: 0 = ok, AC_ERR_ARG (-1) = rejected arguments, AC_ERR_LAUNCH (-2) = HIP launch error.
 *     Nothing throws across the ABI.
 *   - no hidden global state.
 */
#ifndef AUDIOCAPTION_HIP_H
#define AUDIOCAPTION_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AC_OK 0
#define AC_ERR_ARG (-1)
#define AC_ERR_LAUNCH (-2)

#define AC_ABI_VERSION 2
int ac_abi_version(void);

/* ---- log-mel front-end -------------------------------------------------------------------------
 * Replaces torchaudio MelSpectrogram + AmplitudeToDB + transposes + bn0 as called at
 * cnn_encoder.py:418-429 (Cnn14: n_fft 1024, hop 320) / hf_wrapper.py:292-293 (EffB2: n_fft 512, hop 160).
 * wav (B, L) -> out[b*stride_b + t*stride_t + m*stride_m], t < T = L/hop + 1, m < 64;
 * frames T <= t < rows_per_clip are written as 0.  scale/shift (64 each, may be NULL) fold bn0.
 * window [n_fft], twiddle [n_fft] complex (re,im) = exp(-2 pi i n/n_fft), melfb [n_fft/2+1][64],
 * mel_lo/mel_hi [64] = first/last non-zero bin of each filter. */
int ac_logmel(const float* wav, int B, int L, int n_fft, int hop, const float* window, const float* twiddle,
              const float* melfb, const int* mel_lo, const int* mel_hi, const float* scale, const float* shift,
              float* out, int rows_per_clip, long stride_b, long stride_t, long stride_m, void* stream);

/* ---- Cnn14 conv stack ---------------------------------------------------------------------------
 * Activations are channels-last with row padding: [B*Hp][W][C], rows h >= H of every clip are zero
 * (see csrc/conv3x3.hip).  Replaces ConvBlock.forward cnn_encoder.py:59-75 (conv3x3 + eval BN + ReLU
 * [+ avg_pool2d]) and the mean/transposes of cnn_encoder.py:443-444.
 *   mode 0: out [B*Hp][W][Cout]           (conv1 of a block)
 *   mode 1: out [B*Hp/2][W/2][Cout]       (conv2 + 2x2 average pooling)
 *   mode 2: out [B][H][Cout] dense        (last conv2 + mean over the W == 2 mel columns = attn_emb)
 * wpk = weights packed as [Cin/32][9][Cout][32] (chunk, tap = ky*3+kx, out channel, in channel % 32); scale/shift = folded BatchNorm.
 * map_mode: -1 auto, 0 linear, 1 weight-slab-per-XCD, 2 halo-patch-per-XCD block mapping. */
int ac_conv3x3_bn_relu(const float* in, const float* wpk, const float* scale, const float* shift, float* out,
                       int B, int Hp, int H, int W, int Cin, int Cout, int mode, int map_mode, void* stream);
/* Same operation in Winograd F(2x2,3x3) form (2.25x fewer multiplications, fp32): identical arguments
 * except the weights, upk = U = G g G^T packed as [Cin/32][4 j][4 i][Cout][32] (transform column j, row i);
 * Hp must be even. */
int ac_conv3x3_bn_relu_winograd(const float* in, const float* upk, const float* scale, const float* shift,
                                float* out, int B, int Hp, int H, int W, int Cin, int Cout, int mode,
                                int map_mode, void* stream);
/* Same operation on split-bf16 operands ("bf16x3": x = hi + lo in bf16, hi*hi + hi*lo + lo*hi accumulated in
 * f32 on v_mfma_f32_32x32x16_bf16; ~2^-16 relative operand error, 5.3x the f32 matrix rate) - the 1e-3-logit
 * precision tier.  Activations in/out stay f32; wpk = weights split offline and packed as
 * [Cin/32][9][2 (hi, lo)][Cout][32] bf16. */
int ac_conv3x3_bn_relu_bf16x3(const float* in, const void* wpk, const float* scale, const float* shift, float* out,
                              int B, int Hp, int H, int W, int Cin, int Cout, int mode, int map_mode, void* stream);
/* bf16x3 with the weight fragments read straight from L2 (no LDS weight ring, no per-tap barrier):
 * wfrag = split weights in MFMA fragment order [Cin/32][9][2 k-steps][Cout/32][2 (hi, lo)][64 lanes][8] bf16,
 * lane = (cout % 32) + 32 * ((cin % 16) / 8), element = cin % 8. */
int ac_conv3x3_bn_relu_bf16x3_gw(const float* in, const void* wfrag, const float* scale, const float* shift,
                                 float* out, int B, int Hp, int H, int W, int Cin, int Cout, int mode,
                                 int map_mode, void* stream);
/* The same operation (ConvBlock.forward, cnn_encoder.py:59-75) with 1.5x fewer multiplications: 1-D Winograd F(2,3)
 * along the time axis (row pairs) on split-bf16 operands - the input transform V = B^T d (+-1 coefficients) in f32,
 * then hi + lo; the filter transform U = G g evaluated offline in f64, then hi + lo; three bf16 MFMA products per
 * transformed product, f32 accumulation, output transform + BN + ReLU (+ pool / mean) in the epilogue.  Two bf16 MFMA
 * products per f32 product of the direct form (ac_conv3x3_bn_relu_bf16x3_gw: three) at the same f32-grade accuracy.
 * in / out f32 with the layouts of ac_conv3x3_bn_relu.  wfrag = U split and packed in MFMA fragment order
 * [Cin/32][3 kx][4 positions][2 k-steps][Cout/32][2 (hi, lo)][64 lanes][8] bf16, lane = (cout % 32) + 32 * ((cin % 16) / 8),
 * element = cin % 8.  Requires Hp even, W = 2 or a multiple of 4, Cin % 32 == 0, and Cout % 128 == 0 or Cout == 64 with
 * W % 16 == 0 (conv2 of block 1) (AC_ERR_ARG otherwise; mode 1 needs W >= 4, mode 2 needs W == 2), and an input of less
 * than 2 GiB, (B * Hp + 16) * W * Cin * 4 < 2^31 (32-bit byte offsets through one buffer descriptor; AC_ERR_ARG beyond:
 * the caller convolves the batch in clip chunks - the clips of a batch do not interact).
 * Ragged batches (the reference pads every clip to the batch maximum and convolves the padding, collate_func.py:29-32,
 * cnn_encoder.py:446-450): clip_frames (device int32 [B], may be NULL) = every clip's own attn_emb_len; workgroups whose
 * output rows all lie at or beyond need_mul * clip_frames[b] + need_add of their clip(s) skip the convolution and store
 * zeros.  The caller derives (need_mul, need_add) per layer from the receptive field downstream.  With this F(2,3) kernel
 * every output frame below clip_frames[b] - all the temporal encoder reads (model_util.py:10-27) - is then bit-identical
 * to the run that convolves the padding.  The F(4,3) kernels below form a row quad from six input rows: the same
 * (need_mul, need_add) leave valid frames within the tier's own error of the dense run (measured <= 5e-5, token ids
 * equal), and bit-identity needs the wider windows of cnn_encoder.rows_needed(quads=True) (AUDIOCAPTION_RAGGED_EXACT=1). */
int ac_conv3x3_bn_relu_wino1d(const float* in, const void* wfrag, const float* scale, const float* shift,
                              float* out, int B, int Hp, int H, int W, int Cin, int Cout, int mode,
                              int map_mode, const int* clip_frames, int need_mul, int need_add, void* stream);
/* The same layer for launches of a few workgroups (single clips: conv2 of block 6 at B = 1 is 16 workgroups streaming
 * 200 MB of weights): the K loop is cut into slices on separate workgroups, every slice stores its transformed sums to
 * workspace[slice][B*Hp][W][Cout], and a second kernel adds the slices IN ORDER (deterministic) and applies BN / ReLU /
 * pool / mean.  ac_conv3x3_wino1d_splitk_floats: floats of workspace the geometry needs, 0 when the launch is not split
 * (the call then equals ac_conv3x3_bn_relu_wino1d).  clip_frames / need_mul / need_add as above: skipped blocks come out
 * as zeros here too. */
/* The same layer followed by F.dropout(drop_p) on its output (the train-mode forward of the frozen network,
 * cnn_encoder.py:431-442), applied in the epilogue: output element i of the output buffer is scaled by the counter-hash
 * mask ac_dropout(seed, seed_dev) gives index i - bit-identical to the layer followed by ac_dropout over the buffer,
 * without the extra pass over it.  Modes 0 and 1 (the mean over mel of the last block comes after its dropout). */
int ac_conv3x3_bn_relu_wino1d_drop(const float* in, const void* wfrag, const float* scale, const float* shift,
                                   float* out, int B, int Hp, int H, int W, int Cin, int Cout, int mode, int map_mode,
                                   float drop_p, unsigned long long drop_seed, const unsigned long long* seed_dev,
                                   void* stream);
long ac_conv3x3_wino1d_splitk_floats(int B, int Hp, int W, int Cin, int Cout);
int ac_conv3x3_bn_relu_wino1d_splitk(const float* in, const void* wfrag, const float* scale, const float* shift,
                                     float* out, int B, int Hp, int H, int W, int Cin, int Cout, int mode,
                                     int map_mode, const int* clip_frames, int need_mul, int need_add,
                                     float* workspace, long workspace_floats, void* stream);

/* The same layer for FEW PIXELS and heavy weights (conv blocks 5-6 at one to a few clips: conv2 of block 6 is 64 pixels
 * against 151 MB of weights): a K-sliced DIRECT convolution on split-bf16 operands built to stream the weights once at
 * memory bandwidth (csrc/conv3x3_skinny.hip) - 9 taps instead of the 12 / 18 transformed ones, eight fragment groups in
 * flight per wave, all pixels of up to eight 32-pixel tiles per workgroup; the slices' raw sums go to
 * workspace[slice][B*Hp*W][Cout] and a second kernel adds them IN ORDER (deterministic) and applies BN / ReLU / pool /
 * mean and, with drop_p > 0, F.dropout on the output (the mask ac_dropout gives the output buffer; modes 0 and 1).
 * ConvBlock.forward, cnn_encoder.py:59-75 (+ the pooling / mean of :431-444); the arithmetic of
 * ac_conv3x3_bn_relu_bf16x3_gw (2^-16 operand error), wfrag = ITS pack ([Cin/32][9][2][Cout/32][hi, lo][64][8] bf16).
 * W = 4 (modes 0, 1) or 2 (modes 0, 2), Cin % 32 == 0, Cout % 128 == 0, B * Hp * W <= 2048 pixels.
 * ac_conv3x3_skinny_workspace_floats: floats of workspace the geometry needs, 0 when it is not covered (AC_ERR_ARG). */
long ac_conv3x3_skinny_workspace_floats(int B, int Hp, int W, int Cin, int Cout);
int ac_conv3x3_bn_relu_skinny(const float* in, const void* wfrag, const float* scale, const float* shift, float* out, int B,
                              int Hp, int H, int W, int Cin, int Cout, int mode, float* workspace, long workspace_floats,
                              float drop_p, unsigned long long drop_seed, const unsigned long long* seed_dev, void* stream);

/* Second generation of the f32-grade tier: the same layer as a 1-D Winograd F(4,3) along time (row QUADS: 6 transformed
 * positions per 4 output rows, 18 instead of 36 products per (cin, cout)) on split-bf16 operands - 1.5 bf16 MFMA products
 * per f32 product (F(2,3): 2) - with ONE 512-register wave per SIMD (csrc/conv3x3_wino43.hip).  Same layouts, epilogue
 * modes 0 / 1 and ragged-batch arguments as ac_conv3x3_bn_relu_wino1d; replaces the same reference code: ConvBlock.forward,
 * cnn_encoder.py:59-75 (+ the pooling of Cnn14Encoder.forward, :431-441).  Covers the full-width layers W = 32, 16, 8, 4
 * (conv blocks 2-5; modes 0, 1) and W = 2 (block 6: column tiles that skip the taps on the zero padding; modes 0 and
 * 2 = mean over the two mel columns, out (B, H, Cout), cnn_encoder.py:443) with Cout % 128 == 0, Cin % 32 == 0,
 * Hp % 4 == 0; wfrag
 * [Cin/16][3 kx x 6 positions][Cout/32][hi, lo][64 lanes][8] bf16 (U = G g in f64, then split).  tiles_per_wave: 2 (192
 * accumulators, one workgroup per CU), 1 (96 accumulators, <= 256 registers: two workgroups per CU, one's prologue and
 * epilogue under the other's K loop - the short-K layers), or 0 = chosen by the layer's K steps.  The input is
 * addressed through a buffer descriptor rebased per workgroup, so any B * Hp * W * Cin is accepted (B * Hp < 2^23 rows: the
 * epilogue's row -> clip arithmetic; callers chunk clips beyond it).  Ragged batches: see the contract note above - valid
 * frames within 5e-5 of the dense run with the F(2,3) windows, bit-identical with the quad-wide ones.
 * AC_ERR_ARG for shapes outside this list. */
int ac_conv3x3_bn_relu_wino43(const float* in, const void* wfrag, const float* scale, const float* shift, float* out,
                              int B, int Hp, int H, int W, int Cin, int Cout, int mode, int map_mode, int tiles_per_wave,
                              const int* clip_frames, int need_mul, int need_add, void* stream);
/* ... followed by F.dropout in the epilogue (see ac_conv3x3_bn_relu_wino1d_drop). */
int ac_conv3x3_bn_relu_wino43_drop(const float* in, const void* wfrag, const float* scale, const float* shift, float* out,
                                   int B, int Hp, int H, int W, int Cin, int Cout, int mode, int map_mode, float drop_p,
                                   unsigned long long drop_seed, const unsigned long long* seed_dev, void* stream);
/* Workgroups ac_conv3x3_bn_relu_wino43 launches for a geometry at two tiles per wave (0: not covered): callers route
 * launches of a few workgroups (single clips) to the K-sliced F(2,3) form instead. */
long ac_conv3x3_wino43_workgroups(int B, int Hp, int W, int Cout);

/* The row-SEXTET tile form of ac_conv3x3_bn_relu_wino43: F(6,3) along time (points 0, +-1, +-2, +-1/2, inf), 8 transformed
 * positions per 6 output rows = 24 instead of 27 products per (cin, cout) and sextet, 11 % fewer MFMAs per output row,
 * and 1.5 x the rows per workgroup (fewer rounds of workgroups, each paying its prologue and epilogue once).  Same kernel
 * source, arguments, layouts, epilogue modes, tiles_per_wave and ragged-batch arguments as the quad form; the stacked
 * B * Hp rows are one signal with zero rows between clips, so a sextet may straddle two clips and the last one may be
 * cut (Hp % 4 == 0 stays the contract of every buffer; every output row is masked by its own h < H).  Covers W = 32, 16, 8
 * (conv blocks 2-4; modes 0, 1), Cin % 32 == 0, Cout % 128 == 0; wfrag [Cin/16][3 kx x 8 positions][Cout/32][hi, lo]
 * [64 lanes][8] bf16 (U = G g in f64, then split).  The input transform is evaluated in f32 before the split as in the
 * quad form; the larger constants of F(6,3) cost nothing against the 2^-16 operand error (tests/test_wino63_ref_cpu.py).
 * AC_ERR_ARG for shapes outside this list. */
int ac_conv3x3_bn_relu_wino63(const float* in, const void* wfrag, const float* scale, const float* shift, float* out,
                              int B, int Hp, int H, int W, int Cin, int Cout, int mode, int map_mode, int tiles_per_wave,
                              const int* clip_frames, int need_mul, int need_add, void* stream);
/* ... followed by F.dropout in the epilogue (see ac_conv3x3_bn_relu_wino1d_drop). */
int ac_conv3x3_bn_relu_wino63_drop(const float* in, const void* wfrag, const float* scale, const float* shift, float* out,
                                   int B, int Hp, int H, int W, int Cin, int Cout, int mode, int map_mode, float drop_p,
                                   unsigned long long drop_seed, const unsigned long long* seed_dev, void* stream);

/* Conv block 1 at f32 grade in ONE kernel (csrc/conv3x3_block1_w4.hip): conv1 (Cin = 1) + BN + ReLU is computed straight
 * into the staging of conv2, conv2 + BN + ReLU + 2x2 average pool runs as F(4,3) on split-bf16 operands; persistent
 * workgroups (one per CU) walk tiles of 8 rows x 64 columns.  The 64-channel intermediate never exists in HBM.
 * in1 [B*Hp][64] f32 (log-mel after bn0), w1 [64][9], wfrag2 = the F(4,3) pack of conv2 ([4][18][2][hi, lo][64][8] bf16),
 * out [B*Hp/2][32][64] f32.  Hp % 8 == 0.  Replaces ConvBlock.forward of conv_block1 + F.avg_pool2d, cnn_encoder.py:59-75 /
 * :431-432: bit-identical to ac_conv3x3_first followed by ac_conv3x3_block1_conv2_wino43.  clip_frames / need_mul /
 * need_add: ragged batches (see ac_conv3x3_bn_relu_wino1d); drop_p > 0: F.dropout on the pooled output in the epilogue
 * (see ac_conv3x3_bn_relu_wino1d_drop). */
int ac_conv3x3_block1_wino43(const float* in1, const float* w1, const float* scale1, const float* shift1,
                             const void* wfrag2, const float* scale2, const float* shift2, float* out, int B, int Hp,
                             int H, const int* clip_frames, int need_mul, int need_add, float drop_p,
                             unsigned long long drop_seed, const unsigned long long* seed_dev, void* stream);
/* The same kernel with conv1 on the matrix cores as well (the default of the host class): a [32 channels] x [K = 16: nine
 * taps times the BN scale + the BN shift against a constant 1] x [32 columns] split-bf16 product per row, whose result a lane
 * holds in the layout conv2's staging stores - 1760 of the 4700 vector instructions per tile gone for 8 % more MFMAs.  Same
 * arguments; conv1 has the split-bf16 grade of the tier's other layers (not bit-identical to ac_conv3x3_first).
 * cnn_encoder.py:59-75 / :431-432. */
int ac_conv3x3_block1_wino43_mfma(const float* in1, const float* w1, const float* scale1, const float* shift1,
                                  const void* wfrag2, const float* scale2, const float* shift2, float* out, int B, int Hp,
                                  int H, const int* clip_frames, int need_mul, int need_add, float drop_p,
                                  unsigned long long drop_seed, const unsigned long long* seed_dev, void* stream);
/* The conv2 half of the same kernel on a 64-channel input in HBM ([B*Hp][64][64] f32, B*Hp*64*64*4 < 2^31): the unfused
 * form the fused kernel is tested against. */
int ac_conv3x3_block1_conv2_wino43(const float* in64, const void* wfrag2, const float* scale2, const float* shift2,
                                   float* out, int B, int Hp, int H, void* stream);

/* "f16x2" tier of the same kernel.  Activations live in HBM as fp16 (in: [B*Hp][W][Cin] fp16; out: fp16 for modes 0
 * and 1, f32 for mode 2 = the attn_emb the rest of the path consumes), weights as fp16 hi + lo (2^-22) in the same
 * fragment order, two fp16 MFMA products per f32 product, f32 accumulation, fp16 rounding (RNE, 2^-12 relative) once
 * per stored activation.  The caller scales every output channel of the weights by a power of two before splitting
 * (so the lo parts stay normal fp16 numbers) and multiplies `scale` by the inverse.  Same shape arguments and error
 * codes as ac_conv3x3_bn_relu_bf16x3_gw.  Replaces the same reference code: ConvBlock.forward, cnn_encoder.py:318-338.
 * out_f32 != 0 (mode 1 only): the pooled output is written as f32 (it feeds a split-bf16 block: the mixed tier runs
 * conv_block6, K = 9216 / 18432, on ac_conv3x3_bn_relu_bf16x3_gw).  overflow_flag (may be NULL): one device word that is
 * OR-ed with 1 when a value about to be stored as fp16 exceeds the fp16 range (65504) - the caller re-runs the batch
 * on an f32-activation tier instead of returning inf/NaN-poisoned results.
 * AC_ERR_ARG when B*Hp*W*Cin >= 2^32 (32-bit staging offsets). */
int ac_conv3x3_bn_relu_f16x2_gw(const void* in, const void* wfrag, const float* scale, const float* shift,
                                void* out, int B, int Hp, int H, int W, int Cin, int Cout, int mode,
                                int map_mode, int out_f32, unsigned int* overflow_flag, void* stream);
/* Block 1 of the "f16x2" tier in one kernel: conv1 (Cin = 1) + BN + ReLU is computed straight into the LDS patch of
 * conv2 (the 64-channel intermediate never exists in HBM), conv2 + BN + ReLU + 2x2 average pool on the matrix cores.
 * in1 [B*Hp][64] f32 (log-mel after bn0), w1 [64][9], wfrag2 as for ac_conv3x3_bn_relu_f16x2_gw (Cin = Cout = 64),
 * out [B*Hp/2][32][64] fp16.  Replaces ConvBlock.forward of conv_block1, cnn_encoder.py:318-338 / :431. */
int ac_conv3x3_block1_f16x2(const float* in1, const float* w1, const float* scale1, const float* shift1,
                            const void* wfrag2, const float* scale2, const float* shift2, void* out,
                            int B, int Hp, int H, int W, unsigned int* overflow_flag, void* stream);

/* Y[M][N] = act(X[M][K] W[N][K]^T + bias) on the split-bf16 matrix path (2^-16 relative operand error, f32
 * accumulation): the one-tap instance of the "gw" convolution kernel.  X, Y dense row-major f32; wfrag = W split into
 * bf16 hi + lo in fragment order [K/32][1][2 k-steps][N/32][2][64 lanes][8]; ones = N floats of 1.0;
 * K % 32 == 0, N % 64 == 0.  Replaces the same reference code as ac_linear (nn.Linear / the nn.GRU input projections,
 * rnn_encoder.py:34-49) for the large layers. */
int ac_linear_bf16x3(const float* X, const void* wfrag, const float* ones, const float* bias, float* Y,
                     int M, int N, int K, int relu, void* stream);

/* First conv (Cin = 1): in [B*Hp][64], w [64][9] (OIHW), out [B*Hp][64][64]. */
int ac_conv3x3_first(const float* in, const float* w, const float* scale, const float* shift, float* out,
                     int B, int Hp, int H, int W, void* stream);
/* The same with an fp16 output [B*Hp][64][64] (first layer of the "f16x2" tier). */
int ac_conv3x3_first_f16(const float* in, const float* w, const float* scale, const float* shift, void* out,
                         int B, int Hp, int H, int W, unsigned int* overflow_flag, void* stream);

/* ---- Cnn6: 5x5 / stride 1 / pad 2 convolutions (csrc/conv5x5.hip) ---------------------------------
 * Same [B*Hp][W][C] f32 channels-last rows as the 3x3 kernels, with a stronger row rule: a 5x5 conv reads TWO rows beyond
 * a clip, so Hp >= H + 2 and Hp even (AC_ERR_ARG otherwise).  Input rows at or beyond a clip's own H are read as zeros
 * whatever the buffer holds; output rows at or beyond H (H / 2 of a pooled output) are written as zeros.
 * Replace ConvBlock5x5.forward (cnn_encoder.py:96-111) + F.avg_pool2d of Cnn6Encoder.forward (cnn_encoder.py:192-199). */
/* Block 1 (Cin = 1, 25 taps, f32 FMAs) + BN + ReLU + 2x2 average pool in one kernel: in [B*Hp][64] (log-mel after bn0),
 * w [64][25] (OIHW), out [B*Hp/2][32][64]; an odd H loses its last row, as F.avg_pool2d does. */
int ac_conv5x5_first(const float* in, const float* w, const float* scale, const float* shift, float* out,
                     int B, int Hp, int H, void* stream);
/* Implicit GEMM (M = pixels, N = Cout, K = 25 * Cin) on split-bf16 operands: x = hi + lo (RNE both), three
 * v_mfma_f32_32x32x16_bf16 products per f32 product, f32 accumulation - the arithmetic of ac_conv3x3_bn_relu_bf16x3_gw.
 * BN folded to scale / shift on the f32 accumulator, ReLU; mode 0 = full output [B*Hp][W][Cout], 1 = 2x2 average pool
 * (ReLU before the pool) [B*Hp/2][W/2][Cout].  wfrag from ac_pack_conv5x5_weight_bf16x3.  W = 8, 16 or 32, Cin % 32 == 0,
 * Cout % 128 == 0. */
int ac_conv5x5_bn_relu_bf16x3(const float* in, const void* wfrag, const float* scale, const float* shift, float* out,
                              int B, int Hp, int H, int W, int Cin, int Cout, int mode, void* stream);
/* w OIHW f32 [Cout][Cin][5][5] (device) -> wfrag: hi = RNE_bf16(w), lo = RNE_bf16(w - hi) in MFMA fragment order
 * [Cin/32][25 taps][2 k-steps][Cout/32][2 (hi, lo)][64 lanes][8] bf16, lane = (cout % 32) + 32 * ((cin % 16) / 8),
 * element = cin % 8: Cin * Cout * 100 bytes.  Cin % 32 == 0, Cout % 32 == 0. */
int ac_pack_conv5x5_weight_bf16x3(const float* w, void* wfrag, int Cin, int Cout, void* stream);

/* ---- dense projection ---------------------------------------------------------------------------
 * Y[M,N] = act(X[M,K] W[N,K]^T + bias): every F.linear of the path (rnn_encoder.py:41 input
 * projections, transformer_decoder.py:86,95-101).  K % 32 == 0, ldx/ldw % 4 == 0, 16-byte aligned X/W. */
int ac_linear(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K, long ldx,
              long ldw, long ldy, int relu, void* stream);

/* ---- GRU recurrence + pooling -------------------------------------------------------------------
 * One bidirectional layer of the packed GRU (rnn_encoder.py:41 via model_util.py:22-27):
 * gx [B][T][2][3H] = input projections incl. b_ih (gate order r,z,n), whhT [2][H/4][3H][4] = W_hh packed by ac_gru_pack_whh,
 * bhh [2][3H], lens [B] int32; out [B][T][2H], zeros at t >= lens[b].  H must be 256. */
/* packed[d][k/4][n][k%4] = whh[d][n][k] for nn.GRU's weight_hh of both directions, whh [2][3H][H]. */
int ac_gru_pack_whh(const float* whh, float* packed, int hidden, void* stream);
int ac_gru_layer(const float* gx, const float* whhT, const float* bhh, const int* lens, float* out, int B,
                 int T, int hidden, void* stream);
/* The same layer with every (clip, direction) split over FOUR workgroups of 256 threads, each holding its quarter of W_hh
 * in registers for the whole sequence (nothing is re-streamed per step); the parts trade 64 hidden values each per step
 * through L2 as {tag, value} granules (agent-scope relaxed atomics).  whh = nn.GRU's weight_hh of both directions [2][3H][H], NOT
 * packed.  workspace: ac_gru_split_workspace_bytes(B) bytes, 8-byte aligned, owned by the caller; the call clears what
 * it needs (stream-ordered memset).  Its FIRST 4-byte word is a sticky error flag the caller zeroes once: non-zero when
 * a workgroup's partner never started within 2 s (the output is then invalid).  8*B workgroups of 256 threads.
 * save (may be NULL): [B][T][2][4H] = (r, z, n, W_hn h + b_hn) per cell, what ac_gru_layer_bwd needs (ac_gru_layer_train's
 * layout): the training forward. */
long ac_gru_split_workspace_bytes(int B);
int ac_gru_layer_split(const float* gx, const float* whh, const float* bhh, const int* lens, float* out, float* save,
                       void* workspace, int B, int T, int hidden, void* stream);
/* mean_with_lens (model_util.py:41-63); add_max != 0 adds max_with_lens (cnn_encoder.py:451-453). */
int ac_mean_with_lens(const float* x, const int* lens, float* out, int B, int T, int C, int add_max,
                      void* stream);

/* ---- Transformer decoder ------------------------------------------------------------------------
 * Shapes: d_model a multiple of 64 up to 512; nhead divides d_model, head width d_model / nhead <= 64; dim_ff a multiple of
 * 64 up to 512, or a multiple of 512; attn_emb_dim a multiple of 32; 1 <= nlayers <= AC_MAX_LAYERS.  Every entry point below
 * that takes an ac_trm_weights refuses any other shape before it launches anything (AC_ERR_ARG; the size queries: -1). */
#define AC_MAX_LAYERS 8
typedef struct {
  const float *sa_in_w, *sa_in_b, *sa_out_w, *sa_out_b; /* self_attn.in_proj / out_proj       */
  const float *ca_in_w, *ca_in_b, *ca_out_w, *ca_out_b; /* multihead_attn.in_proj / out_proj  */
  const float *l1_w, *l1_b, *l2_w, *l2_b;               /* linear1 / linear2                  */
  const float *n1_w, *n1_b, *n2_w, *n2_b, *n3_w, *n3_b; /* norm1..3                           */
} ac_trm_layer;

typedef struct {
  int32_t d_model, nhead, nlayers, dim_ff, vocab, max_pos, attn_emb_dim, reserved;
  const float* emb;       /* word_embedding.weight [V][d]            */
  const float* pe;        /* pos_encoder.pe        [max_pos][d]      */
  const float* cls_w;     /* classifier.weight     [V][d] (no bias)  */
  const float* proj_w;    /* attn_proj.0.weight    [d][attn_emb_dim] */
  const float* proj_b;    /* attn_proj.0.bias                        */
  const float* proj_ln_w; /* attn_proj.3 (LayerNorm)                 */
  const float* proj_ln_b;
  const float* step_pk;   /* fragment-packed step weights from ac_trm_pack_step_weights */
  ac_trm_layer layer[AC_MAX_LAYERS];
} ac_trm_weights;

/* Row-wise LayerNorm of (x + y) (y may be NULL), eps 1e-5: the post-LN residual blocks of
 * nn.TransformerDecoderLayer and attn_proj's LayerNorm. */
int ac_add_layernorm(const float* x, const float* y, const float* w, const float* b, float* out, int rows,
                     int d, long ldx, long ldy, long ldo, void* stream);

/* Memory side of the decoder, once per batch (transformer_decoder.py:86 + the K/V in-projections of
 * every layer's cross attention, which the reference recomputes on every call):
 *   attn_emb [R*Tm][attn_emb_dim] -> memkv [nlayers][R*Tm][2*d]  (K then V);  tmp: R*Tm*d floats. */
int ac_trm_memory(const ac_trm_weights* w, const float* attn_emb, int R, int Tm, float* memkv, float* tmp,
                  void* stream);

/* The per-position projections read their weights in MFMA fragment order (one contiguous 1 KiB read per
 * wave and fragment).  ac_trm_step_pack_floats = size of that copy; ac_trm_pack_step_weights writes it from
 * the row-major pointers of `w` (w->step_pk itself is not read); the caller then stores `out` in
 * w->step_pk.  Required by ac_trm_greedy / ac_trm_forward_tokens / ac_trm_beam_step; redo it whenever the
 * weights change. */
long ac_trm_step_pack_floats(const ac_trm_weights* w);
int ac_trm_pack_step_weights(const ac_trm_weights* w, float* out, void* stream);

/* Decode-step projection for WIDE row batches (a greedy chain over several submissions, a beam search over grouped batches:
 * 200 ... 1000 rows per step), csrc/decoder_wide.hip:  Y[M][N] = act(P(X)[M][K] W[N][K]^T + bias), the F.linear calls of
 * nn.TransformerDecoderLayer and the classifier (transformer_decoder.py:92-101) with the producer of the A rows fused in -
 * producer 0: X is a fragment PACK of the rows (ac_dec_wide_pack of a [M][K] matrix, or the output of a split_out launch),
 *             K = 256, 512 or 1024, ntb = 1;
 * producer 1: A = emb[tok[r*tok_stride + t]] * emb_scale + pe[t] (transformer_decoder.py:89-91), K = 256;
 * producer 2: A = LayerNorm(X + Y2) * ln_w + ln_b, eps 1e-5 (the post-LN residual join), K = 256.
 * Producers 1 and 2 also store the produced rows to xout (may be NULL).  Arithmetic: both operands split into three bf16 planes
 * (24 significant bits), the six plane products of order <= 2 on v_mfma_f32_32x32x16_bf16 with f32 accumulation - f32-grade
 * (below the rounding of an f32 dot product) at 2.7x the f32 matrix rate.  Pack layout: [tile of 32 rows][k step of 16][plane]
 * [lane = row % 32 + 32 * (k % 16 / 8)][k % 8] bf16, ac_dec_wide_packed_floats(rows, K) floats, 16-byte aligned; Wp = the pack
 * of W.  split_out = 1 (producers 1 / 2, N % 16 == 0): Y receives the PACK of the [M][N] result instead of f32 rows.
 * ntb: 64-column groups per workgroup.  16-byte aligned rows of X / Y2 / xout (Y: any; 16-byte stores when its rows are aligned). */
long ac_dec_wide_packed_floats(int N, int K);
int ac_dec_wide_pack(const float* W, long ldw, int N, int K, float* out, void* stream);
int ac_dec_wide_gemm(int producer, const float* X, long ldx, const float* Y2, long ldy2, const float* ln_w,
                     const float* ln_b, const int* tok, long tok_stride, int t, const float* emb, const float* pe,
                     float emb_scale, float* xout, long ldxo, const float* Wp, const float* bias, float* Y, long ldy, int M,
                     int N, int K, int relu, int ntb, int split_out, void* stream);

/* Number of workspace floats ac_trm_greedy / ac_trm_forward_tokens / ac_trm_beam need. */
long ac_trm_workspace_floats(const ac_trm_weights* w, int rows, int max_len);

/* Greedy decoding (base.py:152-218 stepwise_forward + sample_next_word + stepwise_process_step,
 * transformer_model.py:34-57), fully on device with a self-attention KV cache:
 *   memkv from ac_trm_memory, mem_len [B] int32 (= attn_emb_len),
 *   seq [B][max_len] int64, logit [B][max_len][V], logprob [B][max_len], embed [B][max_len][d];
 *   unfinished_cnt [max_len] int32: rows still unfinished after step t (step t+1.. are the steps the
 *   reference would not have executed once this reaches 0; their seq/logprob columns keep the
 *   reference's initial values end_idx / 0, their logit/embed columns read 0).  ws: ac_trm_workspace_floats(w, B, max_len) floats. */
int ac_trm_greedy(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int Tm, int max_len,
                  int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob,
                  float* embed, int* unfinished_cnt, float* ws, void* stream);

/* ac_trm_greedy over `segments` batches of B / segments rows each in one launch chain (B % segments == 0; rows
 * [i * B / segments, (i + 1) * B / segments) are batch i).  Every batch is searched as if alone: its loop ends when all
 * of ITS rows have emitted <end>, whatever the other batches do.  unfinished_cnt [segments][max_len] int32, row i as
 * ac_trm_greedy's for batch i.  The launch sequence does not depend on the data; once a batch has ended, the workgroups
 * that hold only its rows return at once in every launch of the remaining steps, and the logit / embed columns of the
 * steps a batch did not run read 0 (seq end_idx, logprob 0) - also in ac_trm_greedy and ac_trm_sample, which are this
 * search over one segment. */
int ac_trm_greedy_segments(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int segments, int Tm,
                           int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit,
                           float* logprob, float* embed, int* unfinished_cnt, float* ws, void* stream);

/* The same greedy search (same arguments, same outputs; base.py:152-218, transformer_decoder.py:80-103) as ONE persistent
 * launch for the case that nothing else runs on the GPU (the blocking model() call, single clips): a row is decoded by a
 * cluster of four workgroups for all of its steps - part p owns head p of both attention sub-layers (its keys and values
 * stay in LDS: the projected audio memory of the row and the self-attention cache) and quarter p of the feed-forward
 * units and of the vocabulary; the parts meet in seven exchanges per step (tagged 8-byte granules through L2, the split
 * GRU kernel's hand-off) - csrc/decoder_cluster.hip.  ~45 us per step instead of the launch chain's ~90, for up to two
 * rows per CU; beyond that the clusters run in rounds and ac_trm_greedy is the faster call.  Sums are formed in another
 * order than ac_trm_greedy's (logits equal to ~1e-6, the same token ids on every fixture).
 * cluster_pk: ac_trm_cluster_pack_floats(w) floats written by ac_trm_cluster_pack (per-part weight blobs; redo when the
 * weights change).  workspace: ac_trm_cluster_workspace_bytes(B) bytes, 8-byte aligned; its FIRST 4-byte word is a sticky
 * error flag the caller zeroes once: non-zero when a workgroup's partners never started within 2 s (outputs invalid).
 * early_stop != 0: the launch ends one or two steps after every row has emitted <end> (the reference's loop ends there,
 * base.py:206-211; the columns it would not have written keep their initial values either way); 0: all max_len steps run
 * (what ac_trm_greedy's launches do).
 * Shapes: d_model 256, 4 heads, dim_ff 1024, max_len <= 32, nlayers * (Tm + max_len) * 512 + ~20 KB of LDS <= 160 KB;
 * AC_ERR_ARG otherwise (ac_trm_cluster_pack_floats: -1). */
long ac_trm_cluster_pack_floats(const ac_trm_weights* w);
int ac_trm_cluster_pack(const ac_trm_weights* w, float* out, void* stream);
long ac_trm_cluster_workspace_bytes(int B);
int ac_trm_greedy_cluster(const ac_trm_weights* w, const float* cluster_pk, const float* memkv, const int* mem_len, int B,
                          int Tm, int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit,
                          float* logprob, float* embed, int* unfinished_cnt, void* workspace, int early_stop, void* stream);

/* ---- sampling (base.py:214-252 sample_next_word; stepwise_forward base.py:152-170) -------------
 * method: AC_SAMPLE_PLAIN ("sample" and any name not below: softmax(lp / temp)), AC_SAMPLE_TOPK ("top<k>", k >= 1: the k
 * largest lp, softmax(lp / temp) over them), AC_SAMPLE_TOPP ("top<p>", 0 < p < 1: q = softmax(logit), the shortest prefix of
 * q sorted descending whose mass reaches p, renormalised; temp not used), AC_SAMPLE_GUMBEL ("gumbel": argmax(lp + Gumbel
 * noise) is a draw from softmax(lp); temp does not change the argmax).  lp = log_softmax(logit) in f32.  Ties at the top-k /
 * top-p boundary keep the lower index.  The draw is the inverse CDF in vocabulary order over the kept weights with
 * u = ((x0 >> 8) + 1) * 2^-24, x0 = word 0 of Philox4x32-10 at counter (step, row, 0, 0) and key (seed lo, seed hi): it
 * depends on (seed, row, step) only.  The stored log-probability of the word: lp[w] / temp (plain, top-k: not renormalised),
 * log(q[w] / sum of the kept q) (top-p), lp[w] (gumbel).  seed_dev: ONE uint64 in device memory, read by the kernels (a
 * captured graph replays with the seed the word holds then).  V <= 16384.  AC_ERR_ARG: temp <= 0 (plain, top-k), k < 1 or
 * k > V, p outside (0, 1), unknown method. */
#define AC_SAMPLE_PLAIN 0
#define AC_SAMPLE_TOPK 1
#define AC_SAMPLE_TOPP 2
#define AC_SAMPLE_GUMBEL 3

/* The sampler alone: row r of logit (at logit + r * ld, V words) -> word_out[r] (int32), logprob_out[r], Philox step `step`. */
int ac_sample_rows(const float* logit, long ld, int rows, int V, int method, int k, float top_p, float temp,
                   const uint64_t* seed_dev, int step, int* word_out, float* logprob_out, void* stream);

/* Sampled decoding: ac_trm_greedy's search (same arguments, same outputs, the launch chain) with the token of every step drawn
 * by the sampler above instead of the argmax (base.py:152-170 with sample_method != "greedy"): row b of step t draws with
 * counter (t, b).  Bookkeeping as in greedy decoding: a finished row's seq column is end_idx, its logprob column keeps the
 * drawn word's value (what the reference stores); unfinished_cnt as in ac_trm_greedy. */
int ac_trm_sample(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int Tm, int max_len,
                  int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob,
                  float* embed, int* unfinished_cnt, float* ws, int method, int k, float top_p, float temp,
                  const uint64_t* seed_dev, void* stream);

/* Several sampled captions per clip from ONE memory projection: ac_trm_sample over R = B * samples_per_clip rows, clip-major -
 * row r belongs to clip r / samples_per_clip and reads ITS memory K / V and length, as the rows of a beam do.  memkv (from
 * ac_trm_memory over the B clips) and mem_len have B entries; seq, logit, logprob and embed have R rows; unfinished_cnt
 * [max_len] counts over all R rows (one segment: the search ends when every row has emitted <end>, a row that has ended
 * emits end_idx while its siblings go on).  Row r of step t draws with counter (t, r): by definition the result of
 * ac_trm_sample on the batch with every clip repeated samples_per_clip times and the same seed - bit for bit where the
 * memory projection takes the same kernel for B * Tm rows as for R * Tm (ac_linear: up to 128 rows / beyond), to the
 * last bits of the logits otherwise.  samples_per_clip == 1 is ac_trm_sample.  ws: ac_trm_workspace_floats(w, R, max_len)
 * floats.  AC_ERR_ARG, nothing launched: samples_per_clip < 1, R * (max_len + 1) >= 2^31, and what ac_trm_sample refuses. */
int ac_trm_sample_multi(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int samples_per_clip,
                        int Tm, int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit,
                        float* logprob, float* embed, int* unfinished_cnt, float* ws, int method, int k, float top_p,
                        float temp, const uint64_t* seed_dev, void* stream);

/* Decoder forward on given tokens (teacher forcing / plugin call, transformer_decoder.py:80-103):
 * tokens [N][T] int32; key_mask [N][T] uint8 (1 = masked key, the reference's cap_padding_mask /
 * tgt_key_padding_mask, transformer_model.py:22-23,55) or NULL.  embed [N][T][d], logit [N][T][V]. */
int ac_trm_forward_tokens(const ac_trm_weights* w, const float* memkv, const int* mem_len, int N, int Tm,
                          const int* tokens, const unsigned char* key_mask, int T, float* embed, float* logit,
                          float* ws, void* stream);

/* One beam-search step over R = B*beam rows (base.py:269-289): runs the decoder for position t on
 * tokens[R][max_len+1] / key_mask[R][max_len+1] (column t is the input token; row r uses the audio
 * memory of clip r / beam), forms log_softmax(log_softmax(logit)/temp) + cum_logprob[R] and returns,
 * per clip, the `beam` best candidates over the flattened (beam*V) scores (only the clip's first row at
 * t == 0, base.py:285-289): top_val [B][beam], top_idx [B][beam] (flattened index beam_i*V + word).
 * The self-attention KV cache set (t & 1) of the workspace is the active one. */
int ac_trm_beam_step(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int beam, int Tm,
                     int max_len, int t, float temp, const int* tokens, const unsigned char* key_mask,
                     const float* cum_logprob, float* top_val, int* top_idx, float* ws, void* stream);
/* Per-clip beam bookkeeping on the device (base.py:290-323), one call per step after ac_trm_beam_step: for every clip
 * still active, row k of tokens_out = row (top_idx / V) of tokens_in with the word (top_idx % V) appended at column
 * t + 1 (key_mask_out = tokens_out == pad_idx); beams whose word is end_idx (all of them at t == max_len - 1) are
 * appended, in beam order, to the clip's finished list done_seq [B][done_capacity][max_len] (padded with end_idx) /
 * done_score (= logprob / (t + 1)), their cumulative score gets the reference's -1000; the clip retires when its
 * finished count EQUALS beam (n_active is decremented).  src_row [B*beam] is what ac_trm_beam_reorder needs. */
int ac_trm_beam_update(const float* top_val, const int* top_idx, const int* tokens_in, int* tokens_out,
                       unsigned char* key_mask_out, float* cum_logprob, int* active, int* done_count, int* done_seq,
                       float* done_score, int* src_row, int* n_active, int B, int beam, int V, int max_len, int t,
                       int end_idx, int pad_idx, int done_capacity, void* stream);
/* Re-gather the beams after selection (base.py:294-302): row r of cache set ((t+1) & 1) takes the
 * self-attention KV cache (positions 0..t) of row src_row[r] of set (t & 1). */
int ac_trm_beam_reorder(const ac_trm_weights* w, int R, int max_len, int t, const int* src_row, float* ws,
                        void* stream);

/* The same bookkeeping for a search that never retires a clip (ensemble.py:195-261 has no "enough finished beams" break):
 * every clip stays active to max_len and collects every finished beam - at most beam * max_len, so done_capacity =
 * beam * max_len holds them all.  Same arguments, same kernel; n_active is left alone. */
int ac_trm_beam_update_all(const float* top_val, const int* top_idx, const int* tokens_in, int* tokens_out,
                           unsigned char* key_mask_out, float* cum_logprob, int* active, int* done_count, int* done_seq,
                           float* done_score, int* src_row, int* n_active, int B, int beam, int V, int max_len, int t,
                           int end_idx, int pad_idx, int done_capacity, void* stream);

/* ---- keyword-conditioned decoder (transformer_decoder.py:177-214 KeywordProbTransformerDecoder) -------------
 * A decoder input row becomes LayerNorm(emb[tok] * sqrt(d) + kwp[clip]) * ln_w + ln_b + pe[t] (eps 1e-5) instead of
 * emb[tok] * sqrt(d) + pe[t]; everything after it is the plain decoder's.  kwp [clips][d_model] = keyword_proj(keyword), which
 * the caller computes once per batch (ac_gemm, any keyword width); ln_w / ln_b = word_keyword_norm.  row_div: decoder row r
 * reads kwp row r / row_div - 1 for the greedy, sampled and teacher-forced calls, `beam` for ac_trm_kw_beam_step.  The three
 * pointers are device pointers, 16-byte aligned.  The operands travel as arguments of the launches: stream-ordered, and a
 * captured graph keeps the addresses it was captured with.
 * ac_trm_kw_greedy_segments / _sample / _forward_tokens / _beam_step: their namesakes without `kw_` (same arguments after `kw`,
 * same outputs), always on the launch chain's general / per-row routes.  AC_ERR_ARG before any launch: kw or one of its
 * pointers NULL or misaligned, row_div not the call's.
 * ac_trm_kw_embed_qkv: the first launch of such a step alone, R rows at position t of tokens [R][tok_stride] -
 * xout [R][d_model] the rows as above, qkv [R][3 * d_model] layer 0's self-attention in-projection of them (16-byte aligned). */
typedef struct {
  const float* kwp;
  const float* ln_w;
  const float* ln_b;
  int32_t row_div;
} ac_trm_keyword;
int ac_trm_kw_greedy_segments(const ac_trm_weights* w, const ac_trm_keyword* kw, const float* memkv, const int* mem_len,
                              int B, int segments, int Tm, int max_len, int start_idx, int end_idx, int pad_idx,
                              int64_t* seq, float* logit, float* logprob, float* embed, int* unfinished_cnt, float* ws,
                              void* stream);
int ac_trm_kw_sample(const ac_trm_weights* w, const ac_trm_keyword* kw, const float* memkv, const int* mem_len, int B, int Tm,
                     int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob,
                     float* embed, int* unfinished_cnt, float* ws, int method, int k, float top_p, float temp,
                     const uint64_t* seed_dev, void* stream);
int ac_trm_kw_forward_tokens(const ac_trm_weights* w, const ac_trm_keyword* kw, const float* memkv, const int* mem_len, int N,
                             int Tm, const int* tokens, const unsigned char* key_mask, int T, float* embed, float* logit,
                             float* ws, void* stream);
int ac_trm_kw_beam_step(const ac_trm_weights* w, const ac_trm_keyword* kw, const float* memkv, const int* mem_len, int B,
                        int beam, int Tm, int max_len, int t, float temp, const int* tokens, const unsigned char* key_mask,
                        const float* cum_logprob, float* top_val, int* top_idx, float* ws, void* stream);
int ac_trm_kw_embed_qkv(const ac_trm_weights* w, const ac_trm_keyword* kw, int R, int row_div, int t, const int* tokens,
                        long tok_stride, float* xout, float* qkv, void* stream);

/* ---- ensemble decoding (ensemble.py:94-151 stepwise_forward, :154-276 beam_search) -------------
 * Several captioners decode one batch together: at every step each member's decoder runs on the shared prefix, the word
 * is chosen from m = mean_n log_softmax(logit_n) (f32, NOT renormalised) and is appended for all of them.  The members
 * share tokens / key_mask / unfinished / seq and the vocabulary; each keeps its own weights, audio memory and workspace.
 *
 * ac_trm_step_logits: ONE decoder step for position t over R rows of one member - ac_trm_beam_step's arguments up to the
 * KV-cache set, with row_div in place of beam (row r uses the audio memory of clip r / row_div; R % row_div == 0) and
 * cache_set (0 / 1) naming the active self-attention cache set of the workspace (a greedy or sampled search stays on 0, a
 * beam search alternates t & 1 with ac_trm_beam_reorder).  Writes logit row r at logit + r * ldl (ldl >= V) and, when embed
 * is not NULL, the classifier's input row at embed + r * ld_embed. */
#define AC_ENS_MAX 8
int ac_trm_step_logits(const ac_trm_weights* w, const float* memkv, const int* mem_len, int R, int row_div, int Tm,
                       int max_len, int t, const int* tokens, const unsigned char* key_mask, int cache_set,
                       float* logit, long ldl, float* embed, long ld_embed, float* ws, void* stream);

/* The picks.  logits: n_models (1 .. AC_ENS_MAX, AC_ERR_ARG beyond) HOST pointers to the members' planes, row r of every
 * plane at + r * ld (16-byte aligned planes with ld % 4 == 0 are read with 16-byte loads).  V <= 16384.
 *
 * ac_ens_greedy_pick: word = argmax m (lowest index wins ties); logprob[r][t] = m[word] (ensemble.py:415).  Bookkeeping of
 * ac_trm_greedy on the shared buffers: seq [rows][max_len], tokens / key_mask [rows][max_len + 1] (column t + 1 is
 * written), unfinished [rows], unfinished_cnt [max_len] (zeroed by the caller; the kernel returns at once when
 * unfinished_cnt[t - 1] == 0).  A row that finished before step t emits end_idx and stores no value (the caller's 0 stays) -
 * the reference keeps writing words after <end>; up to and including a row's first <end> the two agree.
 *
 * ac_ens_sample_pick: the sampler of ac_sample_rows / ac_trm_sample over m with ensemble.py:412-449's rules where they
 * depart from base.py: temp divides m before top-p as well; the stored value is m[w] / temp (plain, top-k), the log of the
 * renormalised kept probability (top-p), m[w] (gumbel).  Same Philox counter (t, row) and inverse CDF in vocabulary order.
 * seq != NULL: step t of a search with the bookkeeping above (logprob [rows][max_len]); seq == NULL: the pick alone,
 * word_out[r] and logprob[r].
 *
 * ac_ens_beam_step_select: per row log_softmax(m / temp) + cum_logprob[r], per clip the `beam` best over the flattened
 * (beam * V) scores (only the clip's first row at t == 0): top_val / top_idx [B][beam] as ac_trm_beam_update reads them.
 * beam <= 8; scratch: 2 * B * beam * beam words. */
int ac_ens_greedy_pick(const float* const* logits, int n_models, long ld, int rows, int V, int t, int max_len,
                       int end_idx, int pad_idx, int64_t* seq, float* logprob, int* tokens, unsigned char* key_mask,
                       int* unfinished, int* unfinished_cnt, void* stream);
int ac_ens_sample_pick(const float* const* logits, int n_models, long ld, int rows, int V, int method, int k,
                       float top_p, float temp, const uint64_t* seed_dev, int t, int max_len, int end_idx, int pad_idx,
                       int64_t* seq, float* logprob, int* tokens, unsigned char* key_mask, int* unfinished,
                       int* unfinished_cnt, int* word_out, void* stream);
int ac_ens_beam_step_select(const float* const* logits, int n_models, long ld, int B, int beam, int V, int t, float temp,
                            const float* cum_logprob, float* top_val, int* top_idx, float* scratch, void* stream);

/* ---- group (diverse) beam search (base.py:363-471 diverse_beam_search; csrc/group_beam.hip) -------------
 * G groups of bdash beams per clip, staggered in time: at global step t group g stands at its local position lt = t - g.  A
 * group's step is ac_trm_step_logits over its own B * bdash rows, this selection, ac_trm_beam_update_all (t = lt, beam =
 * bdash) and ac_trm_beam_reorder; the groups of a step run in the order g = 0, 1, ...
 *
 * ac_group_beam_select: logit holds B * bdash rows of V raw logits z at stride ldl >= V.  Per row
 *   lp = log_softmax(log_softmax(z) / temp);  lp[w] -= count[w] * diversity_lambda;  cand = cum[row] + lp
 * where count[w] is the number of rows, among the n_prev * bdash rows of the earlier groups of the same clip, whose word at
 * local position lt is w (the product and the subtraction are each rounded to f32 once; with n_prev == 0 or lambda == 0
 * the scores carry the bits of the un-penalised ones).  prev_tok: a HOST array of n_prev (0 .. AC_GROUP_BEAM_MAX_GROUPS - 1)
 * device pointers, each one earlier group's CURRENT token plane [B * bdash][tok_ld] (column 0 the start token, so column
 * lt + 1 is read; tok_ld >= lt + 2); the pointers are copied into the launch arguments, so a captured graph keeps them.
 * Per clip the bdash best of the flattened bdash * V candidates (only the clip's first row at lt == 0), the lowest flattened
 * index first among equals: top_val / top_idx [B][bdash], beam_i * V + word, as ac_trm_beam_update_all reads them.
 * scratch: 2 * B * bdash * bdash words.  No allocation, no synchronisation.
 * AC_ERR_ARG (nothing is launched): bdash outside 1 .. 8 or above V, n_prev outside 0 .. 7, V outside 1 .. 8192, ldl < V,
 * lt < 0, temp not finite or <= 0, diversity_lambda not finite or < 0, B < 1, a null pointer. */
#define AC_GROUP_BEAM_MAX_GROUPS 8
int ac_group_beam_select(const float* logit, long ldl, int B, int bdash, int V, int lt, float temp,
                         float diversity_lambda, const float* cum, const int* const* prev_tok, int n_prev, long tok_ld,
                         float* top_val, int* top_idx, float* scratch, void* stream);

/* ---- repetition and word constraints of a search (csrc/logit_rules.hip) -------------
 * At step t (0-based) a row has generated g = tokens[1 .. t] - t words, the start token in column 0 is not one of them - and
 * z is its row of raw logits.  In this order:
 *   1. repetition_penalty rho (finite, > 0; 1 = off): for every word w of g, z'[w] = z[w] / rho if z[w] > 0, else z[w] * rho -
 *      computed from z, once per word however often it occurs;
 *   2. no_repeat_ngram n (0 = off): if t >= n - 1, with p the last n - 1 words of g (none for n = 1), every i with
 *      i + n - 1 < t and g[i .. i + n - 2] == p bans the word g[i + n - 1] (overlapping occurrences count);
 *   3. bad_words [n_bad] (device, n_bad <= 256): always banned;
 *   4. min_length: while t < min_length, end_idx is banned.
 * Banned: z'[w] = -inf.  Every pick of this library treats a -inf column as absent and renormalises over the others; a
 * row must keep at least one finite column (the caller's business: the kernel does not count them).
 *
 * ac_logit_rules_apply: rows of z at logit + r * ld_in -> z' at out + r * ld_out, out of place (the planes must not overlap;
 * logit is never written), tokens row r at tokens + r * ld_tok.  One workgroup per row; 16-byte accesses when both planes
 * are 16-byte aligned with strides that are multiples of 4.  No allocation, no synchronisation: capturable.  AC_ERR_ARG,
 * nothing launched: V > 16384, t < 0 or t >= ld_tok, n_bad > 256 (or < 0, or without bad_words), rho not finite or <= 0,
 * negative n or min_length, end_idx outside [0, V), a stride below V, a NULL plane.
 *
 * ac_trm_search_rules: ac_trm_greedy (method = AC_SEARCH_GREEDY; k, top_p, temp, seed_dev unused) or ac_trm_sample_multi
 * (method = AC_SAMPLE_*) over R rows, row_div rows per clip, with the rules between every step's logits and its pick:
 * `logit` [R][max_len][V] keeps the decoder's RAW logits; the constrained row of a step lives in `plane` (R rows of
 * ld_plane >= V floats, overwritten by every step), and logprob holds the constrained distribution's values.
 * ac_trm_beam_step_rules: ac_trm_beam_step with the rules applied to the B * beam rows of raw logits before the scores are
 * formed; plane: B * beam * V floats. */
#define AC_SEARCH_GREEDY (-1)
typedef struct {
  float repetition_penalty;
  int32_t no_repeat_ngram, min_length, end_idx, n_bad;
  const int32_t* bad_words; /* device */
} ac_logit_rules;
int ac_logit_rules_apply(const float* logit, long ld_in, float* out, long ld_out, int rows, int V, const int* tokens,
                         long ld_tok, int t, const ac_logit_rules* rules, void* stream);
int ac_trm_search_rules(const ac_trm_weights* w, const float* memkv, const int* mem_len, int R, int row_div, int Tm,
                        int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob,
                        float* embed, int* unfinished_cnt, float* ws, int method, int k, float top_p, float temp,
                        const uint64_t* seed_dev, const ac_logit_rules* rules, float* plane, long ld_plane, void* stream);
int ac_trm_beam_step_rules(const ac_trm_weights* w, const float* memkv, const int* mem_len, int B, int beam, int Tm,
                           int max_len, int t, float temp, const int* tokens, const unsigned char* key_mask,
                           const float* cum_logprob, float* top_val, int* top_idx, float* ws,
                           const ac_logit_rules* rules, float* plane, void* stream);

/* ---- Bahdanau-attention GRU decoder (rnn_decoder.py:10-36,74-113,159-216, hf_wrapper.py:1377-1554) -------------
 * BahAttnCatFcDecoder / TemporalBahAttnDecoder for inference, csrc/attn_gru.hip.  One GRU layer, unidirectional.  With
 * E = emb_dim, d = d_model, S = attn_size, A = attn_emb_dim, F = fc_emb_dim (each a multiple of 32 up to 1024), V = vocab
 * (<= 16384, the pick and sampling kernels' limit), Tm <= 2048 frames; n_tags = 4 (temporal decoder) or 0.  Every entry
 * point refuses anything else before it launches (AC_ERR_ARG; the size query: -1).
 * One step over R rows (row r uses the audio memory of clip r / row_div), in the reference's order:
 *   score_t = v . tanh(W_h h + ek[t]), -1e10 at t >= len, softmax, c = sum_t w_t attn_emb[t], p_ctx = ctx_proj c,
 *   GRU cell (gates r, z, n) on W_ih[:, :2E] [embed, p_ctx] + gf and W_hh h + b_hh, logit = classifier h' + bias.
 * The projections run on 64-row tiles of the exact-f32 MFMA GEMM (each weight is read once per tile of rows); accurate
 * tanhf / expf.  ek = W_enc attn_emb + b_attn [B][Tm][S] and gf = W_ih[:, 2E:3E] fc_proj(fc_emb) + b_ih [B][3d] do not
 * depend on the step: ac_bah_memory computes them once per batch into the workspace. */
typedef struct {
  int32_t emb_dim, d_model, attn_size, attn_emb_dim, fc_emb_dim, vocab, n_tags;
  int32_t variant;     /* 0: the decoder above; 1 / 2: the condition-controlled decoders below            */
  const float* emb;    /* word_embedding.weight     [V][E]                                      */
  const float* temb;   /* temporal_embedding.weight [4][E] (NULL when n_tags == 0)              */
  const float* w_ih;   /* model.weight_ih_l0        [3d][3E]: columns embed | p_ctx | p_fc      */
  const float* w_hh;   /* model.weight_hh_l0        [3d][d]                                     */
  const float* b_ih;   /* model.bias_ih_l0 [3d]                                                 */
  const float* b_hh;   /* model.bias_hh_l0 [3d]                                                 */
  const float* attn_w; /* attn.h2attn.weight [S][d + A]: decoder-state columns, then the frame's */
  const float* attn_b; /* attn.h2attn.bias   [S]                                                */
  const float* attn_v; /* attn.v             [S]                                                */
  const float* fc_w;   /* fc_proj.weight  [E][F] */
  const float* fc_b;
  const float* ctx_w;  /* ctx_proj.weight [E][A] */
  const float* ctx_b;
  const float* cls_w;  /* classifier.weight [V][d] */
  const float* cls_b;  /* classifier.bias   [V]    */
} ac_bah_weights;

/* Condition-controlled decoders (ConditionalBahAttnDecoder rnn_decoder.py:276-336, SpecificityBahAttnDecoder :519-575): one
 * float per clip, cond (any finite value), in fc_emb's place.  The struct keeps its layout; a slot the variant does not use
 * must be NULL, n_tags 0, and every entry point checks that.
 *   variant 1  GRU input [embed | ctx_proj(c) | (1 - cond) W_c[0] + cond W_c[1]]; fc_w = condition_embedding.weight [2][E],
 *              fc_b NULL.  Only gf differs: W_ih[:, 2E:3E] cond_emb + b_ih.
 *   variant 2  GRU input [embed | c | cond], E + A + 1 wide, no ctx_proj: w_ih = the first E + A columns of weight_ih_l0
 *              repacked to an aligned [3d][E + A] block, fc_w = its last column [3d]; fc_b, ctx_w, ctx_b NULL.
 *              gf = cond W_ih[:, E + A] + b_ih.
 * ac_bah_memory_cond (cond [B] on the device) replaces ac_bah_memory; ac_bah_workspace_floats, ac_bah_step_logits,
 * ac_bah_greedy, ac_bah_sample and ac_bah_beam_gather serve every variant.  The entry points that take fc_emb refuse
 * variants 1 and 2, the _cond ones refuse variant 0 (AC_ERR_ARG). */
int ac_bah_memory_cond(const ac_bah_weights* w, const float* attn_emb, const float* cond, int B, int R, int Tm, int max_len,
                       float* ws, void* stream);
/* Workspace floats of a batch of B clips decoded over R >= B rows (R = B for greedy / sampled search, B * beam for beam
 * search); the same (B, R, Tm, max_len) go to every call that shares the workspace.  16-byte aligned. */
long ac_bah_workspace_floats(const ac_bah_weights* w, int B, int R, int Tm, int max_len);
/* Once per batch: attn_emb [B][Tm][A], fc_emb [B][F] -> ek, gf in ws (the reference recomputes both for every row at every
 * step, hf_wrapper.py:1402,1542). */
int ac_bah_memory(const ac_bah_weights* w, const float* attn_emb, const float* fc_emb, int B, int R, int Tm, int max_len,
                  float* ws, void* stream);
/* ONE decoder step over R = B * row_div rows.  state_in / state_out [R][d] (distinct buffers; zeros before the first step);
 * the input of row r is word id words[r * word_stride] or, with tags != NULL (step 0 of a temporal decoder,
 * hf_wrapper.py:1521-1523), the embedding of tag tags[r / row_div] (0..3).  Writes logit row r at logit + r * ldl (ldl >= V),
 * the GRU output at embed + r * ld_embed (embed may be NULL) and the weight of frame t at
 * attn_weight + r * attn_row_stride + t * attn_frame_stride (may be NULL). */
int ac_bah_step_logits(const ac_bah_weights* w, const float* attn_emb, const int* mem_len, int B, int R, int row_div,
                       int Tm, int max_len, const float* state_in, const int* words, long word_stride, const int* tags,
                       float* state_out, float* embed, long ld_embed, float* logit, long ldl, float* attn_weight,
                       long attn_row_stride, long attn_frame_stride, float* ws, void* stream);
/* Greedy / sampled search (base.py:152-218 with attn_model.py:60-92) in one call, no host synchronisation: max_len times the
 * step plus ac_ens_greedy_pick's / the sampler's pick and bookkeeping.  tags [B] for a temporal decoder, NULL otherwise.
 * seq [B][max_len] int64, logit [B][max_len][V], logprob [B][max_len], embed [B][max_len][d], attn_weight [B][Tm][max_len],
 * state [B][d] (the state after the last executed step), unfinished_cnt [max_len] as ac_trm_greedy's.  Every output is
 * written in full: the columns of a row after its first <end>, and of the steps after every row has ended, read seq = end_idx
 * and 0 everywhere else (the launch sequence does not depend on the data; once the search is over the per-row kernels return
 * at once and the state passes through).  Sampling: ac_trm_sample's rules and Philox counters (step, row). */
int ac_bah_greedy(const ac_bah_weights* w, const float* attn_emb, const int* mem_len, const int* tags, int B, int Tm,
                  int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob,
                  float* embed, float* attn_weight, float* state, int* unfinished_cnt, float* ws, void* stream);
int ac_bah_sample(const ac_bah_weights* w, const float* attn_emb, const int* mem_len, const int* tags, int B, int Tm,
                  int max_len, int start_idx, int end_idx, int pad_idx, int64_t* seq, float* logit, float* logprob,
                  float* embed, float* attn_weight, float* state, int* unfinished_cnt, float* ws, int method, int k,
                  float top_p, float temp, const uint64_t* seed_dev, void* stream);
/* Beam search is ac_bah_step_logits + ac_ens_beam_step_select (one member) + ac_trm_beam_update + this re-gather
 * (hf_wrapper.py:1661,1665-1669): row r of state_next / hist_out takes the new state and the attention history
 * [max_len][Tm] (columns 0..t-1 of hist_in plus step_weight [R][Tm] as column t) of row src_row[r]; the rows of a clip with
 * active_before[clip] == 0 (retired before step t) keep their own.  Distinct in / out buffers. */
int ac_bah_beam_gather(const int* src_row, const int* active_before, const float* state_new, float* state_next,
                       const float* step_weight, const float* hist_in, float* hist_out, int B, int beam, int d, int Tm,
                       int max_len, int t, void* stream);

/* ---- training of the attention-GRU decoder (base.py:131-208 with attn_model.py:34-65; csrc/attn_gru_train.hip) --------
 * The same shapes as above, one row per clip, T = cap.size(1) - 1 steps; every step runs (no early stop).  Step t is the
 * arithmetic of ac_bah_step_logits on the input word  use_cap[t] ? cap[b][t] : (t == 0 ? start_idx : seq[b][t - 1])  (the
 * tag's embedding at t == 0 when tags != NULL), its embedding multiplied by in_dropout's mask: the counter hash of
 * ac_dropout at element index (t * B + b) * E + e with (drop_p, drop_seed, seed_dev).  use_cap is a HOST array of T flags
 * (the scheduled-sampling coins are drawn before anything is launched); cap is int64 [B][cap_ld] on the device, cap_ld >= T.
 * Outputs, written in full: seq [B][T] int64 = the arg-max of every step (first index on ties), logit [B][T][V],
 * logprob [B][T] = max(log_softmax(logit)), embed [B][T][d], attn_weight [B][Tm][T], state [B][d] after the last step.
 * The workspace (ac_bah_train_workspace_floats(w, B, Tm, T) floats, 16-byte aligned; -1: configuration refused) keeps,
 * per (step, clip), the state going in and coming out, W_h h and W_hh h + b_hh, the attention weights, the context, the
 * GRU input, the gates and the input word; tanh(W_h h + ek) is recomputed by the backward, not kept. */
long ac_bah_train_workspace_floats(const ac_bah_weights* w, int B, int Tm, int T);
int ac_bah_train_forward(const ac_bah_weights* w, const float* attn_emb, const float* fc_emb, const int* mem_len,
                         const long long* cap, long cap_ld, const int* use_cap, const int* tags, int B, int Tm, int T,
                         int start_idx, float drop_p, unsigned long long drop_seed, const unsigned long long* seed_dev,
                         int64_t* seq, float* logit, float* logprob, float* embed, float* attn_weight, float* state,
                         float* ws, void* stream);
/* The sampled rollout of self-critical sequence training (rl_model.py:35-38 over base.py:152-170): the chain of
 * ac_bah_train_forward for T = max_length steps with no caption.  Step 0 feeds start_idx (the tag's embedding when tags !=
 * NULL), step t > 0 the word step t - 1 stored in seq; in_dropout's mask index is the same (t * B + b) * E + e.  After the
 * classifier of step t the pick is ac_scst_pick: clip b draws from softmax(log_softmax(logit[b][t]) / temp) with the plain
 * sampler at Philox counter (t, b) under sample_seed_dev (one uint64 on the device), or takes forced[b * forced_ld + t]
 * (forced != NULL: int32 on the device, forced_ld >= T); a clip that has stored end_idx keeps storing end_idx, and every
 * step runs.  seq [B][T] int32 gets the stored words, logprob [B][T] = log_softmax(logit)[word before the rule] / temp;
 * logit, embed, attn_weight, state as ac_bah_train_forward writes them.  scratch: 2 B ints.  The workspace has
 * ac_bah_train_forward's size and layout, so ac_bah_train_backward (same w, attn_emb, fc_emb, mem_len, B, Tm, T and
 * dropout arguments) consumes it unchanged.  AC_ERR_ARG before anything is launched: a NULL pointer (forced may be NULL),
 * T < 1, temp not finite or <= 0, forced_ld < T, tags given to a decoder without tags or missing for one with them, the
 * limits of ac_bah_train_workspace_floats. */
int ac_bah_train_rollout(const ac_bah_weights* w, const float* attn_emb, const float* fc_emb, const int* mem_len,
                         const int* tags, int B, int Tm, int T, int start_idx, int end_idx, float temp,
                         const uint64_t* sample_seed_dev, const int* forced, long forced_ld, float drop_p,
                         unsigned long long drop_seed, const unsigned long long* seed_dev, int* seq, int* scratch,
                         float* logit, float* logprob, float* embed, float* attn_weight, float* state, float* ws,
                         void* stream);
/* Where the backward ADDS the gradient of each tensor of the ac_bah_weights struct - same names and shapes (temb may be NULL when
 * n_tags == 0).  The buffers may be slices of one flat gradient buffer; the caller clears them. */
typedef struct {
  float *emb, *temb, *w_ih, *w_hh, *b_ih, *b_hh, *attn_w, *attn_b, *attn_v, *fc_w, *fc_b, *ctx_w, *ctx_b, *cls_w, *cls_b;
} ac_bah_grads;
/* Backward through time of the forward whose workspace is ws (same w, attn_emb, fc_emb, mem_len, B, Tm, T and dropout
 * arguments; the masks are regenerated), given dlogit [B][T][V].  Per step t = T-1 .. 0: the gate backward, dxin and dctx
 * (exact-f32 products over the B rows), the attention backward - one workgroup per clip, which accumulates the clip's
 * d attn_emb and d(key projection) over the steps by plain read-modify-write (a clip's rows belong to its workgroup and the
 * steps run in stream order) - and the two products into dh_{t-1}.  Off the recurrence, once over all B T rows: dlogit W_cls,
 * every weight gradient and bias column sum, the embedding scatter (word_embedding; temporal_embedding for the tag step).
 * d_attn_emb [B][Tm][A] and d_fc_emb [B][F] are WRITTEN (not added to); frames at or beyond a clip's length get exactly 0. */
int ac_bah_train_backward(const ac_bah_weights* w, const ac_bah_grads* g, const float* attn_emb, const float* fc_emb,
                          const int* mem_len, const float* dlogit, int B, int Tm, int T, float drop_p,
                          unsigned long long drop_seed, const unsigned long long* seed_dev, float* d_attn_emb,
                          float* d_fc_emb, float* ws, void* stream);
/* The same two for variants 1 and 2 (no tags, no rollout): cond [B] instead of fc_emb.  The gradient struct follows the
 * weight struct - unused slots NULL; variant 1: fc_w = where d condition_embedding.weight [2][E] is added; variant 2: w_ih =
 * the gradient of weight_ih_l0 in the parameter's REAL layout [3d][E + A + 1] (not the pack's), fc_w = w_ih + E + A, its
 * last column at row pitch E + A + 1.  cond gets no gradient; d_fc_emb [B][F] is written as zeros. */
int ac_bah_train_forward_cond(const ac_bah_weights* w, const float* attn_emb, const float* cond, const int* mem_len,
                              const long long* cap, long cap_ld, const int* use_cap, int B, int Tm, int T, int start_idx,
                              float drop_p, unsigned long long drop_seed, const unsigned long long* seed_dev, int64_t* seq,
                              float* logit, float* logprob, float* embed, float* attn_weight, float* state, float* ws,
                              void* stream);
int ac_bah_train_backward_cond(const ac_bah_weights* w, const ac_bah_grads* g, const float* attn_emb, const float* cond,
                               const int* mem_len, const float* dlogit, int B, int Tm, int T, float drop_p,
                               unsigned long long drop_seed, const unsigned long long* seed_dev, float* d_attn_emb,
                               float* d_fc_emb, float* ws, void* stream);
/* Backward of fc_emb = mean_with_lens(attn_emb)[:, :F] (rnn_encoder.py:44): d_attn_emb[b][t][c] += d_fc_emb[b][c] / lens[b]
 * for t < lens[b], c < F <= A. */
int ac_bah_mean_lens_bwd(const float* d_fc_emb, const int* lens, float* d_attn_emb, int B, int Tm, int A, int F,
                         void* stream);

/* ---- specificity loss (captioning/losses/loss.py:195-219 SpecificityLossWrapper's condition term; csrc/spec_loss.hip) ----
 * logit [N][T][V] (contiguous), word_spec [V], tgt_len [N] int32 (the caption lengths WITH <eos>: position t counts when
 * t < tgt_len[n] - 1), cond [N].  s[n][t] = sum_v softmax(logit[n][t])_v word_spec[v]; c[n] = sum over the counted t of s,
 * divided by tgt_len[n] - 1 when mean_reduce != 0 (mean_with_lens; the caller refuses tgt_len < 2 there);
 * loss[0] = mean_n (c[n] - cond[n])^2.  Kept for the backward: row_s [N*T] (0 at positions not counted), row_lse [N*T],
 * diff [N] = c - cond.  The backward WRITES dlogit [N][T][V] = g_dev[0] (2 / N) diff[n] scale[n] p_v (word_spec[v] - s),
 * exact zeros in the rows not counted.  No atomics; AC_ERR_ARG for a NULL pointer or a non-positive size. */
int ac_specificity_loss(const float* logit, const float* word_spec, const int* tgt_len, const float* cond, int N, int T,
                        int V, int mean_reduce, float* row_s, float* row_lse, float* diff, float* loss, void* stream);
int ac_specificity_loss_bwd(const float* logit, const float* word_spec, const int* tgt_len, const float* row_s,
                            const float* row_lse, const float* diff, const float* g_dev, int N, int T, int V,
                            int mean_reduce, float* dlogit, void* stream);

/* ---- sound-event tagger (Cnn8rnnSedModel, hf_wrapper.py:1791-1859; csrc/sed.hip) ------------------------------------
 * The tagger's convolutions run on the Cnn14 conv kernels above in mode 0; these entries are what they lack.
 *
 * avg_pool + max_pool of ConvBlock.forward(pool_type="avg+max"), hf_wrapper.py:1212-1215, over a (ph, 2) window (time, mel),
 * ph = 2 or 1, on the row-padded channels-last layout: in [B*Hp][W][C] f32 -> out [B*Hp_out][W/2][C] f32.  Output rows
 * h < H / ph (floor) hold avg + max of their window; rows H / ph <= h < Hp_out are written as zeros (the next conv's zero
 * padding: an odd last input row does not reach them).  mean_w != 0 (ph = 1 only; Hp_out unused): the pool is followed by
 * the mean over the W/2 pooled columns (hf_wrapper.py:1840-1842), out dense [B][H][C].  C % 4 == 0 (16-byte accesses), W
 * even, Hp >= H, Hp_out >= H / ph, in / out 16-byte aligned. */
int ac_pool_avgmax(const float* in, float* out, int B, int Hp, int H, int W, int C, int ph, int Hp_out, int mean_w,
                   void* stream);
/* prob = clamp(sigmoid(x + bias), 1e-7, 1) (hf_wrapper.py:1848) over x [rows][C]; bias [C] or NULL; pre (may be NULL)
 * receives the pre-activation x + bias. */
int ac_sed_head(const float* x, const float* bias, float* pre, float* prob, long rows, int C, void* stream);
/* Cnn8rnnSedModel.forward's host post-processing on the device: double_threshold(framewise, high, low, n_connect) followed
 * by decode_with_timestamps(., time_resolution) (hf_wrapper.py:89-216), where framewise is prob [B][S][C] with every segment
 * repeated `ratio` times and the last one stretched to frames_num >= S * ratio (interpolate + pad_framewise_output,
 * hf_wrapper.py:54-87) - an array this call never forms.  Pass 1, per (clip, class): runs of p > low (f32, strict) that
 * contain a p > high, merged when the gap between two is <= n_connect frames, as (class, onset frame, offset frame).  Pass 2,
 * per clip: segments_to_temporal_tag over all ordered pairs of segments of different classes in the reference's float64
 * arithmetic (t = frame * time_resolution, overlap = e_j - s_k against thre * min(e_j - s_j, e_k - s_k), no contraction),
 * leaving early once both flags are set.  tags [B] int32 = 2 * after + while (-1: the segment list overflowed, which the
 * workspace's worst-case size C * ceil(S / 2) per clip rules out).  Pass 2 is quadratic in a clip's segments: a few
 * hundred segments are microseconds, the (unphysical) worst case of every class alternating in step is seconds.
 * rule: HOST pointer to two doubles {time_resolution, thre} (0.01 and 0.5 in the reference), read before the call returns.
 * workspace: ac_sed_tag_workspace_bytes(B, S, C) bytes, 16-byte aligned; the call clears what it needs. */
long ac_sed_tag_workspace_bytes(int B, int S, int C);
int ac_sed_temporal_tag(const float* prob, int B, int S, int C, int frames_num, int ratio, float high, float low,
                        int n_connect, const double* rule, void* workspace, long workspace_bytes, int* tags, void* stream);

/* ================================== training step ==================================
 * The reference trains GRU + decoder on the frozen Cnn14 with scheduled sampling: step t runs the decoder on a
 * (N, t+1) prefix and keeps the last position's logit (base.py:131-137,152-199, transformer_model.py:34-57).  The
 * host keeps every prefix pass in one row space (row = one token position of one pass); forward kernels work on the
 * row range of a pass, backward kernels on all rows at once.  Dropout masks are a counter hash of
 * (seed, element index) - splitmix64, keep iff the top 32 bits >= p * 2^32, kept values scaled by 1/(1-p) - so the
 * backward regenerates them and the CPU oracle reproduces them.  Every dropout site takes `seed` plus an optional
 * device word `seed_dev`: the effective seed is seed + (*seed_dev << 16), which lets a captured HIP graph draw fresh
 * masks on every replay (the host bumps the device word between replays).                                          */

/* C[M][N] (row pitch ldc) = epi( sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn] ): X W^T / dY W / dY^T X with one kernel
 * (replaces F.linear and its autograd, e.g. transformer_decoder.py:86-101, rnn_encoder.py:41).
 * epi: + bias[n], activation (relu = 1: ReLU, 2: swish x*sigmoid(x), 3: sigmoid), dropout(drop_p, drop_seed, index (row0+m)*N+n),
 * + beta*C.  splitk > 1: K is cut into splitk slices whose partial sums are atomically ADDED to C (weight gradients, and
 * input gradients with few output tiles over a long reduction; beta == 1, or beta == 0: C is zero-filled first; no
 * bias/activation/dropout).  a_scale (optional): A(m,k) is multiplied by
 * a_scale[(m / a_rows)*K + k] on the way in - the squeeze-excite gate of an MBConv block applied inside its 1x1
 * projection (efficientnet_pytorch MBConvBlock.forward; call site hf_wrapper.py:231). */
int ac_gemm(const float* A, long sam, long sak, const float* B, long sbk, long sbn, float* C, long ldc, int M, int N,
            int K, const float* bias, int relu, float beta, int splitk, float drop_p, unsigned long long drop_seed,
            const unsigned long long* seed_dev, long row0, const float* a_scale, int a_rows, void* stream);
/* The same contract on split-bf16 operands: every f32 operand is split into bf16 hi + lo
 * when it is staged (16 significant bits), three bf16 MFMAs per product, f32 accumulation - 2^-16 relative operand error
 * at ~5x the f32 matrix rate.  Used for the large GEMMs of the training step (backward dY W / dY^T X over 7 392 rows,
 * teacher-forced forward).  Operands must be contiguous along k or along their row dimension with 16-byte aligned rows;
 * anything else, and products under ~3e7 multiply-adds or under 200 tiles of 64 x 64, are forwarded to ac_gemm (exact f32). */
int ac_gemm_bf16x3(const float* A, long sam, long sak, const float* B, long sbk, long sbn, float* C, long ldc, int M,
                   int N, int K, const float* bias, int relu, float beta, int splitk, float drop_p,
                   unsigned long long drop_seed, const unsigned long long* seed_dev, long row0, const float* a_scale,
                   int a_rows, void* stream);
/* y[i] = x[i] * mask(seed, idx0 + i): F.dropout (cnn_encoder.py:432-442, nn.GRU inter-layer dropout); applying it to
 * a gradient with the same seed is its backward. */
int ac_dropout(const float* x, float* y, long n, float p, unsigned long long seed, const unsigned long long* seed_dev,
               long idx0, void* stream);
/* g[i] = h[i] > 0 ? g[i] * scale : 0 - backward of dropout(relu(.)) given its output h (FFN hidden). */
int ac_mask_pos_scale(float* g, const float* h, long n, float scale, void* stream);
/* Decoder input tokens of scheduled-sampling step t (transformer_model.py:44-52): word[row0 + n*L + l] =
 * use_cap[t] ? cap[n][l] : (l == 0 ? start_idx : seq[n][l-1]); cap int64 [N][cap_ld], seq int32 [N][seq_ld]. */
int ac_build_prefix(const long long* cap, int cap_ld, const int* seq, int seq_ld, const int* use_cap, int t,
                    int start_idx, int* word, long row0, int N, int L, void* stream);
/* x[row] = dropB(dropA(E[word[row]]) * sqrt(d) + pe[pos[row]]) for rows row0..row0+rows (transformer_decoder.py:88-90;
 * in_dropout and PositionalEncoding's dropout), and its backward into the embedding table (atomic adds, all rows). */
int ac_embed_fwd(const float* emb, const float* pe, const int* word, const int* pos, float* x, long row0, long rows,
                 int d, float pa, unsigned long long seed_a, float pb, unsigned long long seed_b,
                 const unsigned long long* seed_dev, void* stream);
int ac_embed_bwd(const float* dx, const int* word, float* demb, long rows, int d, float pa, unsigned long long seed_a,
                 float pb, unsigned long long seed_b, const unsigned long long* seed_dev, void* stream);
/* The same for a KeywordProbTransformerDecoder (transformer_decoder.py:196-202), d = 256:
 *   x[row] = dropB( LayerNorm( dropA(E[word[row]]) * sqrt(d) + kwp[clip[row]] ) * gamma + beta + pe[pos[row]] ),
 * clip [all rows] int32: the clip (row of kwp = keyword_proj(keyword), [clips][d]) a row belongs to; gamma / beta =
 * word_keyword_norm; the dropout sites and their element index are ac_embed_fwd's.  pre [all rows][d] receives the LayerNorm's
 * input.  The backward (all rows at once) takes dx = d(loss)/dx and ADDS d gamma, d beta, dkwp [clips][d] (the sum over each
 * clip's rows) and the embedding table's gradient (atomic adds); d keyword_proj follows from dkwp by ac_gemm.  emb, pe, kwp,
 * gamma, beta, pre, x, dx: 16-byte aligned. */
int ac_kw_embed_fwd(const float* emb, const float* pe, const int* word, const int* pos, const int* clip, const float* kwp,
                    const float* gamma, const float* beta, float* pre, float* x, long row0, long rows, int d, float pa,
                    unsigned long long seed_a, float pb, unsigned long long seed_b, const unsigned long long* seed_dev,
                    float eps, void* stream);
int ac_kw_embed_bwd(const float* dx, const int* word, const int* clip, const float* pre, const float* gamma, float* dgamma,
                    float* dbeta, float* dkwp, float* demb, long rows, int d, float pa, unsigned long long seed_a, float pb,
                    unsigned long long seed_b, const unsigned long long* seed_dev, float eps, void* stream);
/* pre = res + dropout(x); y = LayerNorm(pre) over d = 256 columns (post-LN residual blocks of
 * nn.TransformerDecoderLayer; attn_proj's Dropout -> LayerNorm with res = NULL, transformer_decoder.py:38-43).
 * xmod > 0: x has only xmod rows and row r reads x[r % xmod] (the projected audio memory is shared by all passes, only
 * its dropout mask differs). */
int ac_dropadd_ln_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* pre, float* y,
                      long row0, long rows, long xmod, int d, float p, unsigned long long seed,
                      const unsigned long long* seed_dev, float eps, void* stream);
/* Backward over rows 0..rows: dpre -> dres (= or += when accumulate), dpre * mask [* (relu_src > 0)] -> dx,
 * dgamma / dbeta accumulated atomically.  dx or dres may be NULL. */
int ac_dropadd_ln_bwd(const float* dy, const float* pre, const float* gamma, float* dx, float* dres, int accumulate,
                      const float* relu_src, long relu_mod, float* dgamma, float* dbeta, long rows, int d, float p,
                      unsigned long long seed, const unsigned long long* seed_dev, float eps, void* stream);
/* Multi-head attention over short sequences (nn.MultiheadAttention inside nn.TransformerDecoderLayer), head_dim 64,
 * one workgroup per (sequence, head).  Sequence s: qlen[s] queries at rows qrow0[s].., klen[s] keys at rows
 * krow0[s]...  Key j is visible to query i iff j < kvalid[s] (if given), j <= i (if causal) and
 * word[krow0[s] + j] != pad_idx (if word given).  P (softmax before dropout) is kept at
 * P[((s*nhead + h)*pl + i)*ptk + j]; that index also drives the attention dropout.  Launch covers sequences
 * seq0 .. seq0+nseq; lmax / tkmax bound qlen / klen over the launch. */
int ac_attn_seq_fwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* o, long ldo,
                    float* P, int pl, int ptk, const int* qrow0, const int* qlen, const int* krow0, const int* klen,
                    const int* kvalid, const int* word, int pad_idx, int causal, int seq0, int nseq, int nhead,
                    int head_dim, int lmax, int tkmax, float drop_p, unsigned long long seed,
                    const unsigned long long* seed_dev, void* stream);
int ac_attn_seq_bwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const float* P, int pl,
                    int ptk, const float* dout, long lddo, float* dq, long lddq, float* dk, long lddk, float* dv,
                    long lddv, const int* qrow0, const int* qlen, const int* krow0, const int* klen, int seq0, int nseq,
                    int nhead, int head_dim, int lmax, int tkmax, float drop_p, unsigned long long seed,
                    const unsigned long long* seed_dev, void* stream);
/* The backward of ac_attn_seq_fwd with the same arguments as ac_attn_seq_bwd, tiled over rows for sequences whose
 * score block does not fit one workgroup (the Transformer encoder's self-attention over T' + 1 rows): one launch of
 * ATT_TILE query rows per workgroup writes dq, one of ATT_TILE key rows per workgroup writes dk / dv.  LDS grows
 * linearly with lmax and tkmax; every (lmax, tkmax) ac_attn_seq_fwd accepts is accepted.  No atomics: the result is
 * the same on every launch.  The dropout mask is regenerated from the P index, as in ac_attn_seq_bwd.  d_ws (optional,
 * nseq*nhead*pl floats of scratch): the query pass stores each row's D = dO . O there for the key pass; without it the
 * key pass recomputes D in every key tile (same result, more work). */
int ac_attn_self_bwd_tiled(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const float* P,
                           int pl, int ptk, const float* dout, long lddo, float* dq, long lddq, float* dk, long lddk,
                           float* dv, long lddv, const int* qrow0, const int* qlen, const int* krow0, const int* klen,
                           int seq0, int nseq, int nhead, int head_dim, int lmax, int tkmax, float drop_p,
                           unsigned long long seed, const unsigned long long* seed_dev, float* d_ws, void* stream);
/* dst[i] = src[index[i]] / dst[index[i]] += src[i] over rows of C floats (classifier on each pass's last position,
 * base.py:181-183). */
int ac_gather_rows(const float* src, const int* index, float* dst, long nrows, int C, void* stream);
int ac_scatter_add_rows(const float* src, const int* index, float* dst, long nrows, int C, void* stream);
/* SpecAugment of the train-mode Cnn14 (torchlibrosa SpecAugmentation as the reference configures it,
 * cnn_encoder.py:352-354,423-425: 2 time stripes of width < 64 frames and 2 mel stripes of width < 8 bins per clip,
 * zeroed before bn0): x [B*rows_per_clip][F] is the bn0-normalised log-mel, stripes [B][n_time + n_freq][2] =
 * (begin, length) drawn on the host; a masked bin is set to fill[mel] = bn0(0) (0 when fill is NULL). */
int ac_specaug(float* x, const int* stripes, const float* fill, int B, int rows_per_clip, int T, int F, int n_time,
               int n_freq, void* stream);
/* out[r] = sum_t x[t*n + r], t < reps (gradient of the projected audio memory shared by all passes). */
int ac_sum_replicas(const float* x, float* out, long n, int reps, void* stream);
/* Cnn14 head when dropout sits between the last block and the mel mean (train mode, cnn_encoder.py:441-444):
 * out[b][h][c] = mean_w x[(b*Hp + h)][w][c] for h < H. */
int ac_rows_mean_w(const float* x, float* out, int B, int Hp, int H, int W, int C, void* stream);
/* dst[b][c][r] = src[b][r][c] (k-major copy of W_hh for the recurrence kernel). */
int ac_transpose(const float* src, float* dst, int batch, int rows, int cols, void* stream);
/* out[n] += sum_m x[m*ld + n] (bias gradients). */
int ac_colsum(const float* x, long ld, float* out, long M, int N, void* stream);
/* out[r*out_ld] = argmax_v logit[r*ld + v], first index on ties (sample_next_word "greedy", base.py:206-209). */
int ac_argmax_rows(const float* logit, long ld, int rows, int V, int* out, long out_ld, void* stream);
/* LabelSmoothingLoss (loss.py:51-74): logit [N][T][V], tgt int64 [N][tgt_ld], tgt_len int32 [N]; row_loss [N*T];
 * loss[0] = inv_count * sum(row_loss); dlogit (optional) = gscale [* gscale_dev[0]] * (softmax - q) on valid rows,
 * 0 elsewhere (gscale_dev: the upstream gradient of the loss when it lives on the device).  inv_count <= 0 /
 * gscale <= 0 mean "1 / sum_n min(tgt_len[n], T)", computed on the device (reduction "mean" inside a HIP graph). */
int ac_label_smoothing_loss(const float* logit, const long long* tgt, long tgt_ld, const int* tgt_len, int N, int T, int V,
                            float smoothing, float inv_count, float* row_loss, float* loss, float* dlogit, float gscale,
                            const float* gscale_dev, void* stream);
/* ---- self-critical sequence training (rl_model.py:24-62; csrc/scst.hip) --------------------------
 * ac_scst_pick: pass t of the training engine's rollout.  Clip n (row n of logit, at logit + n * ld, V <= 16384 words)
 * draws a word with the sampler of ac_sample_rows - AC_SAMPLE_PLAIN, temp, Philox counter (t, n), seed_dev one uint64 in
 * device memory: the draw depends on (seed, n, t) only and equals ac_sample_rows' on the same row - or, with `forced`
 * (int32 [N][forced_ld]), takes forced[n][t].  done [N] (written at t == 0, no need to clear it) carries the finished-row
 * rule (base.py:161-166): once a clip has emitted end_idx every later word is end_idx.  seq[n * seq_ld + t] (int32) gets
 * the word, logprob[n * lp_ld + t] = log_softmax(logit[n])[word before the rule] / temp (base.py:249).  drawn [N]: scratch. */
int ac_scst_pick(const float* logit, long ld, int N, int V, float temp, const uint64_t* seed_dev, int t, int end_idx,
                 const int* forced, long forced_ld, int* done, int* drawn, int* seq, long seq_ld, float* logprob, long lp_ld,
                 void* stream);
/* ac_scst_loss: logit [N][T][V], seq int32 [N][seq_ld], reward f32 [N] in device memory.  mask[n][t] = (t == 0 or
 * seq[n][t-1] != end_idx); row_loss[n*T + t] = -(log_softmax(logit[n][t])[seq[n][t]] / temp) * reward[n] * mask;
 * loss[0] = (1 / N) sum row_loss; dlogit (optional) = [gscale_dev[0] *] (reward[n] * mask / (N * temp)) *
 * (softmax(logit[n][t]) - onehot(seq[n][t])), exactly 0 on masked rows.  V <= 16384, temp > 0 (AC_ERR_ARG otherwise). */
int ac_scst_loss(const float* logit, const int* seq, long seq_ld, const float* reward, float temp, int end_idx, int N, int T,
                 int V, float* row_loss, float* loss, float* dlogit, const float* gscale_dev, void* stream);
/* ac_scst_group_reward: the reward of K rollouts per clip (multi-rollout SCST).  scores f32 [K][N] (rollout k of clip n at
 * k * N + n), reward f32 [K * N] in the same order - the row order of the rollout's decoder batch -, all device memory.
 * mode AC_SCST_BASELINE_GREEDY: reward[k][n] = scores[k][n] - greedy_scores[n] (greedy_scores f32 [N]);
 * mode AC_SCST_BASELINE_MEAN (leave-one-out): reward[k][n] = scores[k][n] - (sum_j scores[j][n] - scores[k][n]) / (K - 1),
 * the sum in f32 in the order j = 0 .. K-1; greedy_scores is not read and may be NULL.  One launch, no allocation, no
 * synchronisation (capturable).  AC_ERR_ARG, nothing launched: K < 1, K > AC_SCST_MAX_ROLLOUTS, the mean mode with K < 2,
 * N < 1, an unknown mode, scores or reward NULL, greedy_scores NULL in the greedy mode. */
#define AC_SCST_MAX_ROLLOUTS 8
#define AC_SCST_BASELINE_GREEDY 0
#define AC_SCST_BASELINE_MEAN 1
int ac_scst_group_reward(const float* scores, int K, int N, int mode, const float* greedy_scores, float* reward,
                         void* stream);
/* ---- token-level knowledge distillation (kd_loss.py:8-49; csrc/kd.hip) ------------------------------
 * ac_kd_loss: SupKdLoss(LabelSmoothingLoss(smoothing), TokenLevelKdLoss(temp, "kl"), sup_weight) in one pass per row.
 * logit / tchr_logit [N][T][V] (student / frozen teacher), tgt int64 [N][tgt_ld], tgt_len int32 [N].  On a valid row
 * (t < tgt_len[n]) row_sup[n*T + t] is ac_label_smoothing_loss' row term and row_kd[n*T + t] =
 * -sum_v softmax(tchr / temp)_v * log_softmax(logit / temp)_v (not scaled by temp^2, as the reference); a masked row gets
 * 0 in both and neither logit row is read there (NaN at a teacher's padded positions stays out).
 * loss[1] = inv_count * sum(row_sup), loss[2] = inv_count * sum(row_kd), loss[0] = sup_weight * loss[1] +
 * (1 - sup_weight) * loss[2].  dlogit (optional) = gscale [* gscale_dev[0]] * [sup_weight * (softmax(logit) - q) +
 * (1 - sup_weight) * (softmax(logit / temp) - softmax(tchr / temp)) / temp] on valid rows, exactly 0 elsewhere; with
 * sup_weight == 1 the teacher's values do not enter it.  inv_count <= 0 / gscale <= 0: "1 / sum_n min(tgt_len[n], T)" on
 * the device, as in ac_label_smoothing_loss.  2 <= V <= 16384, temp finite and > 0, 0 <= sup_weight <= 1 (AC_ERR_ARG
 * otherwise). */
int ac_kd_loss(const float* logit, const float* tchr_logit, const long long* tgt, long tgt_ld, const int* tgt_len, int N,
               int T, int V, float smoothing, float temp, float sup_weight, float inv_count, float* row_sup, float* row_kd,
               float* loss, float* dlogit, float gscale, const float* gscale_dev, void* stream);
/* ---- encoder-level knowledge distillation (kd_wrapper.py:56-226, hf_wrapper.py:1095-1111; csrc/enc_kd.hip) ----------
 * ac_enc_kd_loss: the loss head of MseEncoderKdWrapper / ContraEncoderKdWrapper / ContraMseEncoderKdWrapper behind the two
 * projections, forward and backward in f32 (replaces F.normalize, the similarity product, the two F.cross_entropy, F.mse_loss
 * and their autograd: kd_wrapper.py:105-109, 147-155, 210-224).  s [B][ld_s] / t [B][ld_t]: the student's / teacher's
 * projected embedding, width D; kind = AC_ENC_KD_CONTRA and / or AC_ENC_KD_MSE, AC_ENC_KD_L2NORM = the MSE term on the
 * normalised rows (l2_norm=True).  With n(x) = x / max(||x||_2, 1e-12):
 *   loss[1] = 0.5 * (CE(L, diag) + CE(L^T, diag)), each a mean over B, L = logit_scale[0] * n(s) n(t)^T (logit_scale is one
 *             float in device memory, used as it is, not exponentiated); 0 without AC_ENC_KD_CONTRA;
 *   loss[2] = mean over B*D of (a - b)^2, (a, b) = (n(s), n(t)) with AC_ENC_KD_L2NORM, (s, t) without; 0 without AC_ENC_KD_MSE;
 *   loss[0] = loss[1] + loss[2].
 * ds / dt [B][D] (dense) and dscale[1] (each optional) are WRITTEN with gscale [* gscale_dev[0]] times the gradient of
 * loss[0]; dscale[0] = 0 without AC_ENC_KD_CONTRA.  A row below the 1e-12 clamp gets dy / 1e-12; a row is normalised once
 * (kd_wrapper.py:216 normalises a second time, which changes neither value nor gradient above the clamp).  The soft-maxes
 * are max-subtracted.  No atomics (bit-identical on every call), no host synchronisation, at most four launches (two
 * without AC_ENC_KD_CONTRA).  1 <= B <= 512, 1 <= D <= 4096, ld_s, ld_t >= D, any 4-byte aligned base pointers, gscale
 * finite; everything else is AC_ERR_ARG before anything is launched.  ws: ac_enc_kd_workspace_floats(B, D) floats (-1 for a
 * B or D out of range), owned by the caller. */
#define AC_ENC_KD_CONTRA 1
#define AC_ENC_KD_MSE 2
#define AC_ENC_KD_L2NORM 4
long ac_enc_kd_workspace_floats(int B, int D);
int ac_enc_kd_loss(const float* s, long ld_s, const float* t, long ld_t, int B, int D, int kind, const float* logit_scale,
                   float* loss, float* ds, float* dt, float* dscale, float gscale, const float* gscale_dev, float* ws,
                   void* stream);
/* ---- CIDEr-D on token ids (csrc/cider.hip): the SCST reward without a trip through the host -----------------------
 * The metric as pycocoevalcap's cider_scorer.py computes it (n-grams of 1 .. order words, order = 4 and sigma = 6 there;
 * document frequencies counted over the keys of THIS call's references, hypotheses not counted):
 *   df[g] = keys with g in at least one reference;  idf[g] = log(keys) - log(max(1, df[g]));
 *   vec[n][g] = tf(g) * idf[g] per sentence, norm[n] = |vec[n]|, length = max(words - 1, 0);
 *   val[n] = sum over g in h of min(vec_h[n][g], vec_r[n][g]) * vec_r[n][g], divided by norm_h[n] * norm_r[n] when both
 *   are non-zero (and held to <= 1, its bound in exact arithmetic), times exp(-(length_h - length_r)^2 / (2 sigma^2));
 *   score of a key = 10 * mean_n(sum over its references of val[n]) / references.
 * hyp: HOST array of `sets` (<= AC_CIDER_MAX_SETS) device pointers, each int32 [N][hyp_ld], T <= AC_CIDER_MAX_HYP_WORDS
 * words per row.  The sentence of a row (model_util.py:117-164): start_idx skipped, cut at the first end_idx, each word w
 * (0 <= w < vocab_size, else the scores are NaN - never a read) replaced by canon[w], the first id that spells the same
 * word.  Rows of one key are scored once, on row first_row[key] (keys distinct keys, row_key [N] the key of each row).
 * References: ref_words [total_words] canonical ids below n_words (vocab_size + the words outside the vocabulary),
 * sentence s = ref_words[sent_off[s] .. sent_off[s + 1]) with at most max_ref_words <= AC_CIDER_MAX_REF_WORDS words
 * (the caller's maximum over sent_off, checked here before anything is launched; a longer sentence found on the device
 * turns every score into NaN instead), key k owns sentences key_off[k] .. key_off[k + 1], at least one.  All of them in
 * device memory.  workspace: 256-byte aligned, the number of bytes the workspace query returns for the same sizes.
 * scores f32 [sets][N]; reward (optional, sets >= 2) f32 [N] = scores[0] - scores[1].  Integer document frequencies
 * through a table that stores whole n-grams (by the position of one occurrence) and compares them; every float sum has a
 * fixed order: a call is bitwise repeatable.  AC_ERR_ARG beyond any limit, nothing launched. */
#define AC_CIDER_MAX_SETS 4
#define AC_CIDER_MAX_HYP_WORDS 1024
#define AC_CIDER_MAX_REF_WORDS 1024
long ac_cider_workspace_bytes(long ref_words, int sentences, int keys, int sets);
int ac_cider_scores(const int* const* hyp, int sets, long hyp_ld, int N, int T, int start_idx, int end_idx,
                    const int* canon, int vocab_size, int n_words, const int* ref_words, long total_words,
                    const int* sent_off, int sentences, int max_ref_words, const int* key_off, int keys,
                    const int* row_key, const int* first_row, int order, float sigma, void* workspace,
                    long workspace_bytes, float* scores, float* reward, void* stream);
/* ---- BLEU and ROUGE-L on token ids (csrc/capmetrics.hip): the other two string metrics of the reference's evaluation --
 * Both read what ac_cider_scores reads, under the same limits (AC_CIDER_MAX_*) and the same sentence rule: hyp, canon,
 * ref_words / sent_off / key_off / row_key / first_row as described there; a hypothesis word outside [0, vocab_size)
 * turns the scores of its key (and the totals over the keys) into NaN and is never used as an index; reference words
 * are only compared.  workspace: 256-byte aligned, ac_capmetrics_workspace_bytes(keys, sets) bytes, for either entry.
 * Every count is an integer, float64 enters in the closed formulas below and in one sum of fixed order: a call is
 * bitwise repeatable.  AC_ERR_ARG beyond any limit, nothing launched.
 *
 * ac_bleu_scores - pycocoevalcap's bleu_scorer.py with option "closest", n-grams of 1 .. order (<= 4) words, per key:
 *   testlen = hypothesis words;  guess[k] = max(0, testlen - k);
 *   correct[k] = sum over the distinct hypothesis (k+1)-grams of min(count in the hypothesis, max over the key's
 *   references of the count in that reference), whole n-grams compared word by word;
 *   reflen = the reference length closest to testlen, of two equally close the smaller;
 *   b_k = prod_{j <= k} (correct[j] + 1e-15) / (guess[j] + 1e-9);  bleu_k = b_k^(1 / (k + 1)), times exp(1 - 1 / ratio)
 *   when ratio = (testlen + 1e-15) / (reflen + 1e-9) < 1.
 * stats int32 [sets][keys][2 + 2 * order] = testlen, reflen, guess[order], correct[order] (all -1 for a NaN key);
 * scores f64 [sets][order][N], the rows of a key sharing the score of first_row[key]; corpus f64 [sets][order]: the same
 * formulas on the integer totals of the four quantities over the distinct keys.
 *
 * ac_rouge_l_scores - pycocoevalcap's rouge.py, beta = 1.2, per key: lcs(h, r) the longest common subsequence in words of
 * the hypothesis and each reference (the full dynamic program, bit-parallel over 64 hypothesis positions per word: no
 * length heuristic, no band, no cut-off), p = max_r lcs / len(h), r = max_r lcs / len(r) (the two maxima may come from
 * different references), score = (1 + beta^2) p r / (r + beta^2 p) when both are non-zero, else 0.
 * lcs int32 [sets][sentences] (-1 in a NaN key); scores f64 [sets][N]; mean f64 [sets] over the distinct keys. */
long ac_capmetrics_workspace_bytes(int keys, int sets);
int ac_bleu_scores(const int* const* hyp, int sets, long hyp_ld, int N, int T, int start_idx, int end_idx,
                   const int* canon, int vocab_size, const int* ref_words, long total_words, const int* sent_off,
                   int sentences, int max_ref_words, const int* key_off, int keys, const int* row_key,
                   const int* first_row, int order, void* workspace, long workspace_bytes, int* stats, double* scores,
                   double* corpus, void* stream);
int ac_rouge_l_scores(const int* const* hyp, int sets, long hyp_ld, int N, int T, int start_idx, int end_idx,
                      const int* canon, int vocab_size, const int* ref_words, long total_words, const int* sent_off,
                      int sentences, int max_ref_words, const int* key_off, int keys, const int* row_key,
                      const int* first_row, void* workspace, long workspace_bytes, int* lcs, double* scores, double* mean,
                      void* stream);
/* ---- Diversity of a set of captions on token ids (csrc/diversity.hip): Self-BLEU, distinct n-grams, richness ----------
 * hyp: ONE plane of device memory, int32 [N][hyp_ld], T (1 .. AC_CIDER_MAX_HYP_WORDS) words per row, 2 <= N,
 * N * T <= 2^26.  The sentence of a row follows the rule of ac_cider_scores: start_idx skipped, cut at the first end_idx,
 * each word w range-checked against [0, vocab_size) and then replaced by canon[w] (device, int32 [vocab_size]); a word
 * outside the range is never used as an index and makes EVERY float output of the call NaN and every integer output -1.
 * With c_i(g) the occurrences of n-gram g (n = 1 .. 4) in sentence i of L_i words:
 *   Self-BLEU of sentence i = nltk's sentence_bleu(all other sentences, sentence i, weights 1/4 each, smoothing method1):
 *     num[n] = sum over the distinct g of i of min(c_i(g), max_{j != i} c_j(g));  den[n] = max(1, L_i - n + 1 or 0);
 *     ref_len = the length among the OTHER sentences closest to L_i, of two equally close the smaller;
 *     0 when num[1] == 0; else bp * exp(sum_n 0.25 * log(p[n])), p[n] = num[n] / den[n], or 0.1 / den[n] when num[n] == 0,
 *     bp = 1 when L_i > ref_len, else exp(1 - ref_len / L_i);
 *   richness[n] = mean over the sentences with an n-gram of (mean over the sentence's distinct g of log(1 / (docs(g) / N))),
 *     docs(g) the sentences that contain g (NaN when no sentence has an n-gram); richness = sum_n richness[n] * 0.25.
 * Outputs, all in device memory:
 *   stats         int32 [N][10] = L_i, ref_len, den[4], num[4]
 *   sent_distinct int32 [N][4]  = distinct n-grams of sentence i, n = 1 .. 4
 *   totals        int32 [5]     = total words, distinct n-grams of the corpus for n = 1 .. 4
 *   self_bleu     f64 [N]
 *   summary       f64 [6]       = mean Self-BLEU, richness[1 .. 4], richness
 * workspace: 256-byte aligned, ac_diversity_workspace_bytes(N, T) bytes (a multiple of 256; AC_ERR_ARG beyond the limits
 * above).  Whole n-grams are compared word by word in one table, every count is an integer, float64 enters in the closed
 * formulas above and in sums of fixed order: a call is bitwise repeatable.  AC_ERR_ARG beyond any limit, nothing launched. */
long ac_diversity_workspace_bytes(int N, int T);
int ac_diversity_scores(const int* hyp, long hyp_ld, int N, int T, int start_idx, int end_idx, const int* canon,
                        int vocab_size, void* workspace, long workspace_bytes, int* stats, int* sent_distinct, int* totals,
                        double* self_bleu, double* summary, void* stream);
/* ---- Diversity WITHIN groups of captions (csrc/diversity.hip): the captions of one clip scored against each other ------
 * ac_diversity_scores with one more input: group_off, device int32 [G + 1], 0 = group_off[0] <= ... <= group_off[G] = N;
 * rows [group_off[g], group_off[g + 1]) are group g (ragged groups allowed).  "The others" of sentence i are the other
 * sentences OF ITS GROUP, in num[n], in ref_len and everywhere else; the table of distinct n-grams is still one table for
 * the call, with the group as a part of an n-gram's identity: the same words in two groups hold two slots and never count
 * as each other's references.  hyp, T, the sentence rule, canon and the out-of-range rule as in ac_diversity_scores.
 * Outputs, all in device memory:
 *   stats         int32 [N][10], sent_distinct int32 [N][4], self_bleu f64 [N]   as defined for ac_diversity_scores
 *   mbleu         f64 [N][4]    column k - 1 = nltk's sentence_bleu(the others, sentence i, weights 1/k each over the orders
 *                               1 .. k, smoothing method1): 0 when num[1] == 0, else bp * exp(sum_{n <= k} (1 / k) * log(p[n]))
 *                               over the SAME num / den / ref_len integers, so mbleu[i][3] == self_bleu[i] bit for bit
 *   group_totals  int32 [G][5]  = words of the group, distinct n-grams of the group for n = 1 .. 4 (div-n of a clip is
 *                               group_totals[g][n] / group_totals[g][0])
 *   group_mean    f64 [G][5]    = mean of mbleu[.][0 .. 3] over the group's sentences, then their mean Self-BLEU
 *   summary       f64 [5]       = the means of group_mean over the groups, in the order of the groups
 * Richness is not part of the grouped call (its document frequencies are a property of the pooled corpus).
 * Every group needs two rows or more (a single sentence has no "other"): G < 1 or G > N / 2 is AC_ERR_ARG, and callers that
 * hold the offsets on the host check them there (audiocaption_amd/diversity.py).  On the device the offsets are
 * range-checked before they index anything: offsets that are not ascending from 0 to N make every output NaN / -1; a group
 * of fewer than two rows gets NaN / -1 for itself and its rows (and so for summary), and nothing outside it is read.
 * workspace: 256-byte aligned, ac_diversity_group_workspace_bytes(N, T, G) bytes.  Integer counts, float64 in closed formulas
 * and sums of fixed order, every probe bounded by the table size: bitwise repeatable.  AC_ERR_ARG: nothing launched. */
long ac_diversity_group_workspace_bytes(int N, int T, int G);
int ac_diversity_group_scores(const int* hyp, long hyp_ld, int N, int T, int start_idx, int end_idx, const int* canon,
                              int vocab_size, const int* group_off, int G, void* workspace, long workspace_bytes,
                              int* stats, int* sent_distinct, double* self_bleu, double* mbleu, int* group_totals,
                              double* group_mean, double* summary, void* stream);
/* ac_gru_layer that also keeps (r, z, n, W_hn h + b_hn) per (clip, step, direction): save [B][T][2][4H]. */
int ac_gru_layer_train(const float* gx, const float* whhT, const float* bhh, const int* lens, float* out, float* save,
                       int B, int T, int hidden, void* stream);
/* Backward through time of one bidirectional layer (autograd of nn.GRU under pack_padded_sequence,
 * model_util.py:10-27): dout/out [B][T][2H], whh [2][3H][H] -> gate gradients dgx (input side), dgh (hidden side)
 * [B][T][2][3H] and the previous hidden state of every step hprev [B][T][2][H]; weight gradients are GEMMs on those. */
int ac_gru_layer_bwd(const float* dout, const float* out, const float* save, const float* whh, const int* lens,
                     float* dgx, float* dgh, float* hprev, int B, int T, int hidden, void* stream);
/* Optimiser on flat buffers (run.py:122-126, torch.optim.Adam with L2 weight decay, cnn14rnn_trm.yaml:42-46):
 * norm_state[0] += sum g^2;  ac_clip_coef: [1] = sqrt([0]) / grad_div (total norm of the averaged gradient),
 * [2] = min(1, max_norm / (norm + 1e-6)) / grad_div (max_norm <= 0: no clipping);  ac_scale_by_coef: x *= [2];
 * ac_adam_step: g' = g * [2] (norm_state may be NULL) + wd * p, then Adam's update for 1-based `step`. */
/* norm_state has AC_NORM_STATE_FLOATS = 1032 floats, zero-initialised: [0..3] as described here, the rest is scratch of
 * ac_grad_sumsq (per-workgroup partials summed in a fixed order, so that every rank of a data-parallel job gets the
 * same bits); [3] is set to 1 by ac_clip_coef when the gradient norm is not finite, and ac_adam_step
 * then leaves parameters and moments untouched (the reference's NaN-loss skip, run.py:123, without a host sync).
 * ac_swa_update: avg += (p - avg) / (n_averaged + 1) (AveragedModel.update_parameters, train_util.py:233-253;
 * n_averaged = 0 copies). */
int ac_swa_update(float* avg, const float* p, long n, int n_averaged, void* stream);
int ac_grad_sumsq(const float* g, long n, float* norm_state, void* stream);
int ac_clip_coef(float* norm_state, float max_norm, float grad_div, void* stream);
int ac_scale_by_coef(float* x, long n, const float* norm_state, void* stream);
int ac_adam_step(float* p, const float* g, float* m, float* v, long n, const float* norm_state, float lr, float beta1,
                 float beta2, float eps, float weight_decay, int step, const int* step_dev, void* stream);
/* step_dev (may be NULL): the number of updates APPLIED so far, kept on the device; when given, the bias correction
 * uses *step_dev + 1 instead of `step`.  ac_adam_commit advances it after the ac_adam_step launches of one optimiser
 * step - unless norm_state[3] says the update was skipped (the reference does not call optimizer.step() then,
 * run.py:123, so its step count does not advance either). */
int ac_adam_commit(int* step_dev, const float* norm_state, void* stream);

/* ============================ EfficientNet-B2 encoder ============================
 * Replaces efficientnet_pytorch==0.7.1 EfficientNet.extract_features as the reference calls it (hf_wrapper.py:229-241,
 * cnn_encoder.py:798-839; construction restated in eff_latent_encoder.py:74-186).  PARITY UNPINNED: that package is
 * not vendored, the kernels follow its published algorithm.  Activations are channels-last [clip][time][mel][C] fp32
 * (time = the reference's W axis, mel = its H axis).  The 1x1 convolutions are ac_gemm (BatchNorm folded into the
 * weight rows, swish in the epilogue, the squeeze-excite gate as a_scale, the residual as beta = 1).               */

/* 1x1 convolution over channels-last rows: y[M][N] = act((x[M][K] .* gate[m / gate_rows][K]) w[N][K]^T + bias) + beta*y
 * (_expand_conv / _project_conv / _conv_head of efficientnet_pytorch with BatchNorm folded into w and bias; act 0 none,
 * 1 ReLU, 2 swish; gate = the squeeze-excite gate or NULL; beta = 1 adds the block input in place).  K % 8 == 0,
 * N % 4 == 0, 16-byte aligned pointers. */
int ac_pointwise_conv(const float* x, const float* w, const float* bias, float* y, long M, int N, int K, int act, float beta,
                      const float* gate, int gate_rows, void* stream);
/* AmplitudeToDB(top_db) on a (batch, mel, time) tensor: x = max(x, max(x over the WHOLE buffer) - top_db)
 * (hf_wrapper.py:279; torchaudio packs the batch axis as channels).  scratch: >= 1 float (<= 1024 used). */
int ac_top_db_clamp(float* x, long n, float top_db, float* scratch, int scratch_floats, void* stream);
/* Stem: 3x3 stride-2 conv of the 1-channel log-mel x [B][T][F] with w [C][3 mel][3 time], static "same" padding
 * (pad_before / pad_after zeros on both axes), BN scale/shift, swish -> y [B][To][Fo][C]. */
int ac_effnet_stem(const float* x, const float* w, const float* scale, const float* shift, float* y, int B, int T, int F,
                   int C, int pad_before, int pad_after, void* stream);
/* Depthwise k x k conv (k = 3 / 5, stride 1 / 2) + BN + swish: x [B][T][F][C], w [k time][k mel][C] ->
 * y [B][To][Fo][C], To = (T + pad_before + pad_after - k) / stride + 1; pool [B][C] += pool_scale * sum of y over
 * positions (the squeeze of the squeeze-excite layer: pool_scale = 1 / (To*Fo) gives the mean; zero it first). */
int ac_effnet_depthwise(const float* x, const float* w, const float* scale, const float* shift, float* y, float* pool,
                        float pool_scale, int B, int T, int F, int C, int k, int stride, int pad_before, int pad_after,
                        void* stream);
/* gate[b][c] = sigmoid(w2 swish(w1 (pool[b] * inv_count) + b1) + b2), w1 [S][C], w2 [C][S]. */
int ac_effnet_se_gate(const float* pool, float inv_count, const float* w1, const float* b1, const float* w2,
                      const float* b2, float* gate, int B, int C, int S, void* stream);
/* 1x1 convolution / linear layer with static weights on the split-bf16 matrix path (csrc/pw_gemm.hip), the same contract
 * as ac_pointwise_conv: y[M][N] = act((x[M][K] .* gate[m / gate_rows][K]) w^T + bias) + beta * y, for the matrix-bound
 * layers (thousands of rows against hundreds of channels).  The weights are split into bf16 hi + lo and laid out in MFMA
 * fragment order ONCE by ac_pw_gemm_pack (w [N][K] f32 -> wfrag, ac_pw_gemm_packed_bytes(N, K) bytes, 16-byte aligned);
 * activations are split when staged; three bf16 MFMAs per product, f32 accumulation (2^-16 relative operand error).
 * K % 4 == 0, N % 4 == 0, act 0 none / 1 ReLU / 2 swish, 16-byte aligned pointers. */
long ac_pw_gemm_packed_bytes(int N, int K);
int ac_pw_gemm_pack(const float* w, void* wfrag, int N, int K, void* stream);
int ac_pw_gemm_bf16x3(const float* x, const void* wfrag, const float* bias, float* y, long M, int N, int K, int act,
                      float beta, const float* gate, int gate_rows, void* stream);
/* The same with row strides (ldx, ldy in floats, multiples of 4) and inverted dropout on the output (mask = the counter
 * hash of ac_gemm: element index (row0 + m) * N + n, seed + (*seed_dev << 16)): the training step's x W^T (+ bias, ReLU,
 * dropout) and dy W (beta = 1) products (run.py:77-148 through transformer_model.py:20-32), whose weights change every
 * iteration - ac_pw_gemm_pack_strided packs W(n, k) = w[n * s_n + k * s_k] (W^T for the input-gradient product), and
 * ac_pw_gemm_pack_table repacks a whole device-resident table of layers in ONE launch: `count` records
 * {const float* w; void* wfrag; long s_n; long s_k; int N; int K;} (40 bytes each). */
int ac_pw_gemm_bf16x3_ex(const float* x, long ldx, const void* wfrag, const float* bias, float* y, long ldy, long M, int N,
                         int K, int act, float beta, const float* gate, int gate_rows, float drop_p,
                         unsigned long long drop_seed, const unsigned long long* seed_dev, long row0, void* stream);
int ac_pw_gemm_pack_strided(const float* w, long s_n, long s_k, void* wfrag, int N, int K, void* stream);
int ac_pw_gemm_pack_table(const void* table, int count, void* stream);
/* The same gate with the second matrix transposed, w2t [S][C] (= _se_expand.weight^T): one launch per block, both
 * phases read their weights with coalesced 16-byte loads.  C % 4 == 0, 16-byte aligned pointers. */
int ac_effnet_se_gate_t(const float* pool, float inv_count, const float* w1, const float* b1, const float* w2t,
                        const float* b2, float* gate, int B, int C, int S, void* stream);
/* MBConv head in one kernel (csrc/effnet_fused.hip): _expand_conv + _bn0 + swish -> _depthwise_conv + _bn1 + swish ->
 * squeeze sums, the expanded tensor staying in LDS.  x [B][T][F][Cin]; we [Cmid][Cin] / be [Cmid] = the expand
 * convolution with BatchNorm folded in (as for ac_pointwise_conv); wd [k time][k mel][Cmid], scale / shift [Cmid] = the
 * depthwise convolution and its folded BatchNorm (as for ac_effnet_depthwise); y [B][To][Fo][Cmid] (NULL: only the
 * squeeze sums); pool [B][Cmid] += pool_scale * sum of y over positions (zero it first).  Cin % 8 == 0, Cmid % 4 == 0,
 * k = 3 / 5, stride 1 / 2, 16-byte aligned pointers.  AC_ERR_ARG when one input row band does not fit the LDS budget
 * (the caller then runs the two-kernel chain). */
int ac_effnet_expand_depthwise(const float* x, const float* we, const float* be, const float* wd, const float* scale,
                               const float* shift, float* y, float* pool, float pool_scale, int B, int T, int F, int Cin,
                               int Cmid, int k, int stride, int pad_before, int pad_after, void* stream);

/* ===================================== waveform ingest =====================================
 * B clips stored back to back in src (float16 when src_half, else float32; clip b = src[src_off[b] .. src_off[b+1]))
 * -> out [B][lmax] float32: converted, resampled by the windowed-sinc polyphase filter of
 * torchaudio.functional.resample (call site caption_dataset.py:110-120; kernel [new][2*width + orig] with the non-zero
 * tap range [tap_lo, tap_hi) of each phase; orig / new are the gcd-reduced rates; orig == new: conversion only) and
 * zero-padded (WavPadCollate, inference.py:81-111).  out_len[b] = samples of the RESAMPLED clip; out_start[b] (may be NULL
 * = 0) = its first sample kept: output sample o is resampled sample o + out_start[b], zero where that is >= out_len[b] -
 * the random crop / zero pad to audio_duration of caption_dataset.py:121-129 (the caller draws the offsets).  The filter
 * bank is pinned by tests/golden/g13_resample.npz (an independent float64 evaluation of torchaudio 0.13.1's published
 * windowed-sinc prototype on the fine grid; torchaudio itself is not vendored). */
int ac_ingest_resample(const void* src, int src_half, const long* src_off, const float* kernel, const int* tap_lo,
                       const int* tap_hi, float* out, const int* out_len, const int* out_start, int B, int lmax, int orig,
                       int new_, int width, void* stream);

/* ============================== HTS-AT encoder (transformer_encoder.py:679-996), csrc/htsat.hip ==============================
 * A Swin Transformer over the log-mel folded into a 256 x 256 image.  Its linear layers run on ac_gemm / ac_gemm_bf16x3 and its
 * pre-norm LayerNorms on ac_add_layernorm; the entry points below are everything else.  Tokens are row-major over (image
 * row / 4, image column / 4), activations [B][H*W][C] f32.  Every entry point refuses a geometry it does not cover
 * (AC_ERR_ARG) before it launches anything.
 *
 * Patch embedding in one kernel: x = the bn0-normalised log-mel rows of ac_logmel, [B][T][64] dense, T <= 1024.  T < 1024: the time axis is stretched to 1024 frames with torch's bicubic (align_corners,
 * A = -0.75, clamped borders; transformer_encoder.py:940-941); frame f, mel m is image row (f / 256) * 64 + m, column
 * f % 256 (:944-949); then the 4x4 / stride 4 convolution w [C][16] + bias and LayerNorm (:209-220).  out [B][4096][C],
 * C <= 256; w 16-byte aligned. */
int ac_htsat_patch_embed(const float* x, int B, int T, const float* w, const float* bias,
                         const float* ln_w, const float* ln_b, float* out, int C, void* stream);
/* (Shifted-)window attention over 8 x 8 windows, heads of width 24 (C = 24 * heads), H and W multiples of 8:
 * qkv [B][H*W][3C] (q, k, v of all heads per token) -> out [B][H*W][C].  shift (0 .. 7; > 0 needs H, W > 8): the window grid
 * lies on the image rolled by -shift along both axes (gathered and scattered by addressing), and scores between tokens of
 * different regions of the rolled image (:500-519) get -100.  softmax(q k^T / sqrt(24) + bias[head] + mask) v with
 * bias [heads][64][64] = relative_position_bias_table[relative_position_index] (:424-427), gathered by the caller once per
 * weight pack.  Exact-f32 matrix products.  Replaces :411-442 and :533-555. */
int ac_swin_window_attn(const float* qkv, const float* bias, float* out, int B, int H, int W, int C, int heads, int shift,
                        void* stream);
/* PatchMerging without its reduction (:592-601): out [B][H/2*W/2][4C] = LayerNorm over the concatenation of x(2i, 2j),
 * x(2i+1, 2j), x(2i, 2j+1), x(2i+1, 2j+1); H, W even, 4C <= 1536. */
int ac_swin_patch_merge(const float* x, const float* ln_w, const float* ln_b, float* out, int B, int H, int W, int C,
                        void* stream);
/* The tail (:903-912): x [B][Hh*Ww][C] (after the final LayerNorm); token row k * fbins + f is frequency bin f of time chunk
 * k.  attn [B][(Hh/fbins)*Ww][C]: frame k * Ww + w = mean over f; fc [B][C] = mean over all frames (not masked by length). */
int ac_htsat_pool(const float* x, float* attn, float* fc, int B, int Hh, int Ww, int C, int fbins, void* stream);
/* out [B][C] = mean over the N tokens of x [B][N][C]: the layer_i embeddings (:888-897). */
int ac_htsat_token_mean(const float* x, float* out, int B, int N, int C, void* stream);
/* y[i] = x[i] * Phi(x[i]), the exact (erf) GELU of Mlp (:228-243); y may be x. */
int ac_gelu(const float* x, float* y, long n, void* stream);

/* Diagnostic (bench.py, not the hot path): `blocks` workgroups of 4 waves each issue iters x 32 dependent-free
 * v_mfma_f32_32x32x16_bf16 (8 accumulators per wave, no memory traffic); out[blocks * 256] receives the accumulator sums.
 * FLOPs = blocks * 4 * iters * 32 * 32768.  Timed by the caller, it gives the matrix rate the part sustains at the clock it
 * holds under matrix load - the context of `roofline.frac`, whose denominator is the NOMINAL dense peak. */
int ac_mfma_bf16_probe(float* out, int blocks, int iters, void* stream);

/* Diagnostic (tests): the split-bf16 operand split exactly as the kernels apply it (csrc/ac_split_bf16.h).  x [n] f32,
 * n % 4 == 0 -> hi [n / 2], lo [n / 2] dwords of two bf16 each (element 2 i in the low half): hi = RNE_bf16(x),
 * lo = RNE_bf16(x - hi).  One thread per four floats. */
int ac_split_bf16_probe(const float* x, long n, unsigned* hi, unsigned* lo, void* stream);

/* Diagnostic: `blocks` workgroups of `threads` threads record where they ran - out[2 b] = XCC_ID register, out[2 b + 1] =
 * HW_ID register (cu_id bits 11:8, sh_id bit 12, se_id bits 15:13) - and stay resident for spin_ticks of the 100 MHz clock. */
int ac_placement_probe(int* out, int blocks, int threads, int spin_ticks, void* stream);

/* A HIP stream restricted to n_cus compute units (hipExtStreamCreateWithCUMask, mask bits first_cu .. first_cu + n_cus - 1).  The throughput
 * mode (TransformerModel.forward_async) runs its latency-bound decode chains on such a stream: their small workgroups are
 * packed onto a few CUs instead of each holding a CU that a one-workgroup-per-CU conv kernel of the encoder stream then
 * cannot use.  The only entry points of this library that create / destroy a driver object; the caller owns the stream. */
int ac_stream_create_cu_mask(int first_cu, int n_cus, void** out);
int ac_stream_destroy(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AUDIOCAPTION_HIP_H */
