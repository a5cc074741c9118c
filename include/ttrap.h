/*
 * ttrap.h -- C ABI of libttrap_hip.so, the MI355X (gfx950) implementation of the Timbre-Trap
 * hot path:  NSGT constant-Q transform (forward / inverse)  ->  2-D strided-conv autoencoder
 * (forward / backward)  ->  reconstruction / transcription / consistency losses  ->  clip + AdamW.
 *
 * The reference (sony/timbre-trap) is pure Python on stock torch ops and has no FFI of its own;
 * each entry point below names the reference Python it replaces (file:line under /root/reference).
 * The host side that binds these symbols is timbre-trap_amd/timbre_trap/_hip.py (ctypes); the
 * reference-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is DEVICE memory owned by the caller (torch tensors), contiguous, fp32 unless
 *     stated; nothing is allocated or retained by the library; kernels are enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream) and the call returns immediately.
 *   - return value: 0 = ok, >0 = hipError_t of the failed launch, <0 = TT_E_* argument error.
 *   - activations are NCHW with W = time contiguous:  (B, C, H, T).
 *   - no CPU fallback exists: without the library the Python layer raises.
 */
#ifndef TTRAP_H
#define TTRAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TT_E_BADARG      (-1)
#define TT_E_UNSUPPORTED (-2)   /* shape outside the compiled set, or one clip of >= 2^31 elements (32-bit offsets) */

/* flags of tt_resblock_fwd / tt_resblock_bwd: round the operands of the 3x3 convolutions and of dW1 to bf16 for the
 * matrix cores (v_mfma_f32_16x16x32_bf16, fp32 accumulation, fp32 tensors in HBM) at C >= 16.  Default 0 = exact fp32. */
#define TT_FLAG_BF16_OPERANDS 1
/* split-bf16 ("bf16x3"): every fp32 operand is fed to the same instruction as hi + lo (two round-to-nearest bf16) and
 * products are accumulated as hi*hi + lo*hi + hi*lo in fp32 -- fp32-class results (product error ~1e-5 relative,
 * unbiased) at 16/3 of the fp32 matrix rate.  Takes precedence over TT_FLAG_BF16_OPERANDS. */
#define TT_FLAG_BF16_SPLIT    2

#define TT_ACT_NONE 0
#define TT_ACT_ELU  1
/* the output nonlinearities of the magnitude variants' decoders (version 8): TimbreTrapMag.decode's relu (modules.py:976),
 * TimbreTrapMagDB.decode's sigmoid (modules.py:1043); tt_conv2d only */
#define TT_ACT_RELU    2
#define TT_ACT_SIGMOID 3

/* Library / build identification. */
int         tt_version(void);
const char* tt_arch(void);               /* "gfx950" */
const char* tt_error_string(int code);   /* hipGetErrorString for code > 0 */
/* Test / tuning knob (no reference counterpart): the persistent kernels launch min(work items, CUs * workgroups per CU)
 * workgroups with CUs = 256 on MI355X.  A smaller figure makes every workgroup walk several tiles even on small inputs,
 * which is how the parity tests reach the multi-tile loops (cross-tile LDS-DMA prefetch, XCD-ordered tile walk) at sizes
 * the CPU oracle finishes in seconds.  cus <= 0 only queries.  Returns the previous value.  Process-wide, not stream-ordered. */
int         tt_set_cu_limit(int cus);

/* ------------------------------------------------------------------------------------------------
 * NSGT constant-Q transform.  Replaces cqt_pytorch.CQT.encode / .decode as called from
 * timbre_trap/framework/cqtwrapper.py:67 and :207, fused with CQT.to_real (:74-97) /
 * CQT.to_complex (:99-120) and the inf-norm of CQT.decode (:209-211).
 *
 * Specialised for the reference configuration: block_length N = 66150 (3 s @ 22.05 kHz,
 * N/2 = 33075 = 675 * 49), max_window_length M = 1024.  All conventions of the transform are
 * data (tables built on the host by timbre_trap/framework/nsgt_plan.py):
 *   tw675   [675]   float2  exp(-2 pi i j / 675)
 *   tw49    [49]    float2  exp(-2 pi i j / 49)
 *   twNc    [49][675] float2  exp(-2 pi i n2 k1 / 33075)   (four-step twiddles, row n2, column k1)
 *   twN     [33076] float2  exp(-2 pi i j / 66150)
 *   tw1024  [1024]  float2  exp(-2 pi i j / 1024)
 *   bin_tab [F][4]  int32   {spec_start, pad, length, win_off} per bin
 *   window  [sumL]  float   ragged analysis windows   (forward)
 *   dual    [sumL]  float   ragged synthesis windows  (inverse)
 *   gat_off [33077] int32 , gat_idx [sumL] int32   CSR: spectral index -> ragged positions
 *
 * Alignment (every tt_cqt_* entry point, the any-length and Griffin-Lim ones included; tests/test_gpu_cqt_abi_parity.py holds it):
 * `scratch` is 256-byte aligned and every table of a plan 16-byte aligned.  Entry points of csrc/cqt.hip: audio in either direction
 * (audio, daudio, audio_init, audio_out) 8 bytes -- it moves as pairs of samples; coefficients WRITTEN (out of tt_cqt_forward /
 * tt_cqt_forward_mag, dcoeffs of tt_cqt_inverse_bwd) 16 bytes; coefficients READ (coeffs, dcoeffs of tt_cqt_forward_bwd) 4 bytes as
 * planes, 8 as interleaved complex; dmag, mag and conv 4 bytes.  Entry points of csrc/cqt_generic.hip: 4 bytes everywhere, 8 for
 * interleaved complex coefficients.  A scratch or data pointer that breaks its rule is refused with TT_E_BADARG before the first launch.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float*   tw675;
    const float*   tw49;
    const float*   twNc;
    const float*   twN;
    const float*   tw1024;
    const int32_t* bin_tab;
    const float*   window;
    const float*   dual;
    const int32_t* gat_off;
    const int32_t* gat_idx;
    int32_t        n_bins;     /* F */
    int32_t        sum_len;    /* sum of window lengths */
} tt_cqt_plan;

/* bytes of scratch the two calls below need for `n_clips` = B * n_blocks block-clips; 0 for n_clips, n_bins or sum_len <= 0, as
 * tt_cqt_griffin_lim_scratch_bytes.  tt_cqt_generic_scratch_bytes: 0 for n_clips <= 0, -1 for a plan the entry points refuse. */
int64_t tt_cqt_scratch_bytes(int n_clips, int n_bins, int sum_len);

/* audio (B, 1, n_blocks*66150) -> out (B, 2, F, n_blocks*1024), ch0 = re, ch1 = im.
 * If out_complex != 0 the output is interleaved complex64 (B, 1, F, n_blocks*1024) instead
 * (CQT.encode, used raw by experiments/sonify.py:94). */
int tt_cqt_forward(const tt_cqt_plan* plan, const float* audio, float* out, void* scratch,
                   int B, int n_blocks, int out_complex, void* stream);

/* The magnitude variants' encoder input (version 8; TimbreTrapMag.encode, modules.py:948: to_magnitude(sliCQ(audio)).unsqueeze(-3)):
 * audio (B, 1, n_blocks*66150) -> out (B, 1, F, n_blocks*1024) = |c|, written by the band kernel's epilogue -- the two coefficient
 * planes never reach memory.  Same values as tt_magnitude of tt_cqt_forward's output. */
int tt_cqt_forward_mag(const tt_cqt_plan* plan, const float* audio, float* out, void* scratch, int B, int n_blocks, void* stream);

/* coeffs (B, 2, F, n_blocks*1024) [or interleaved complex (B,1,F,T) if in_complex] ->
 * audio (B, 1, n_blocks*66150).  normalize != 0 applies cqtwrapper.py:209-211
 * (divide the whole tensor by its abs-max when that is non-zero) with no host round trip.  The abs-max propagates non-finite
 * values as torch's max does: a NaN sample in any clip makes it NaN and the whole batch comes out NaN, an infinite one divides by inf. */
int tt_cqt_inverse(const tt_cqt_plan* plan, const float* coeffs, float* audio, void* scratch,
                   int B, int n_blocks, int in_complex, int normalize, void* stream);

/* The same transform for ANY block length N and frame count M = 2^m (csrc/cqt_generic.hip): the reference constructor takes
 * arbitrary secs_per_block / sample_rate (timbre_trap/framework/cqtwrapper.py:15-48, cqt_pytorch.CQT(block_length=...,
 * power_of_2_length=True) at :31-35); the two entry points above cover N = 66150 / M = 1024 only.  Slow path by design: the
 * length-N DFT as a Bluestein convolution over P = 2^p >= 2N - 1 points, global-memory Stockham passes, one launch per pass.
 * Tables (host-built, timbre_trap/framework/nsgt_plan.py; bin_tab / window / dual / gat_* as above):
 *   chirp   [N]    float2  exp(-i pi n^2 / N)
 *   bfilt   [P]    float2  DFT_P of the wrapped conjugate chirp, divided by P
 *   twP     [P/2]  float2  exp(-2 pi i q / P)          twM [M/2] float2  exp(-2 pi i q / M)
 *   pos_bin [sumL] int32   bin of every ragged window position
 * Same layouts, flags and normalisation rule as tt_cqt_forward / tt_cqt_inverse (non-finite samples under normalize included: a NaN
 * anywhere in the batch is the peak). */
typedef struct {
    const float*   chirp;
    const float*   bfilt;
    const float*   twP;
    const float*   twM;
    const int32_t* bin_tab;
    const float*   window;
    const float*   dual;
    const int32_t* gat_off;    /* [N/2 + 2] */
    const int32_t* gat_idx;
    const int32_t* pos_bin;
    int32_t        n_bins;
    int32_t        sum_len;
    int32_t        N;
    int32_t        M;
    int32_t        P;
} tt_cqt_gplan;

int64_t tt_cqt_generic_scratch_bytes(const tt_cqt_gplan* plan, int n_clips);
int tt_cqt_generic_forward(const tt_cqt_gplan* plan, const float* audio, float* out, void* scratch,
                           int B, int n_blocks, int out_complex, void* stream);
int tt_cqt_generic_inverse(const tt_cqt_gplan* plan, const float* coeffs, float* audio, void* scratch,
                           int B, int n_blocks, int in_complex, int normalize, void* stream);

/* Adjoints of the transform (version 19): what autograd needs of CQT.encode / the raw synthesis, which the reference inherits as
 * differentiable torch code from cqt_pytorch.  Both directions are real-linear and every window lies inside the open positive
 * half-spectrum, so with a gradient w.r.t. complex values held as dL/dre + i dL/dim (torch's convention), N = block length and
 * M = frames per block:
 *   tt_cqt_forward_bwd   daudio  = (N / 2M) * synthesis of dcoeffs on the ANALYSIS windows (no inf-norm)
 *   tt_cqt_inverse_bwd   dcoeffs = (2M / N) * analysis of daudio on the SYNTHESIS windows
 * The same launches on the same bytes as the direction they run, the constant folded into a scaling that direction already does;
 * layouts and the *_complex flags as in tt_cqt_forward / tt_cqt_inverse (dcoeffs takes the place of coeffs / out).  Fixed summation
 * orders, no atomics: bit-identical from run to run.  Scratch: tt_cqt_scratch_bytes / tt_cqt_generic_scratch_bytes as above. */
int tt_cqt_forward_bwd(const tt_cqt_plan* plan, const float* dcoeffs, float* daudio, void* scratch,
                       int B, int n_blocks, int in_complex, void* stream);
int tt_cqt_inverse_bwd(const tt_cqt_plan* plan, const float* daudio, float* dcoeffs, void* scratch,
                       int B, int n_blocks, int out_complex, void* stream);
/* Gradient of tt_cqt_forward_mag: audio (B, 1, n_blocks*66150) as given to the forward, dmag (B, 1, F, n_blocks*1024) -> daudio.  The
 * band kernel recomputes c in registers, forms dc = dmag c / |c| (exactly 0 where |c| == 0, torch's norm backward) and transforms it
 * in the same wave: neither the coefficients nor their gradient reach memory. */
int tt_cqt_forward_mag_bwd(const tt_cqt_plan* plan, const float* audio, const float* dmag, float* daudio, void* scratch,
                           int B, int n_blocks, void* stream);
int tt_cqt_generic_forward_bwd(const tt_cqt_gplan* plan, const float* dcoeffs, float* daudio, void* scratch,
                               int B, int n_blocks, int in_complex, void* stream);
int tt_cqt_generic_inverse_bwd(const tt_cqt_gplan* plan, const float* daudio, float* dcoeffs, void* scratch,
                               int B, int n_blocks, int out_complex, void* stream);

/* Phase retrieval for the magnitude variants (version 20): audio from |c| by the Griffin-Lim iteration with the momentum of "fast
 * Griffin-Lim" (Perraudin, Balazs, Sondergaard 2013).  The reference has no counterpart: TimbreTrapMag / TimbreTrapMagDB
 * (modules.py:892-1075) return magnitudes, CQT.decode (cqtwrapper.py:184-213) needs complex coefficients, and experiments/sonify.py:109
 * / :158 (audio_rec = model.sliCQ.decode(reconstruction)) therefore serves the complex model only; this entry is the way back for the
 * other two, under the same inf-norm (cqtwrapper.py:209-211).
 *   mag (B, 1, F, n_blocks*1024) target magnitudes, taken as given (no clamp, no non-finite guard)
 *   audio_init (B, 1, n_blocks*66150) the start x_0 (e.g. the input mixture: "mixture phase"), never written; NULL = silence
 * Iteration k = 0 .. n_iter-1, all enqueued by the one call with no host synchronisation:
 *   c = analysis(x_k);  p = mag c / |c|, and mag + 0i where |c| == 0 (a silent start is the zero-phase synthesis; no 0 / 0);
 *   y_k = synthesis(p);  x_{k+1} = y_k + momentum (y_k - y_{k-1}),  x_1 = y_0
 * The synthesis is linear, so the audio-domain extrapolation equals the usual coefficient-domain one t_k = p_k + momentum (p_k - p_{k-1}).
 * One wave per (bin, block-clip) analyses, projects and transforms back in registers: neither c nor p reaches memory.
 *   audio_out = y_{n_iter-1}, the synthesis of a projection; normalize != 0 divides it by its inf-norm exactly as tt_cqt_inverse does
 *   conv (n_iter, B) or NULL: conv[k][b] = sqrt(sum (|c| - mag)^2 / sum mag^2) over clip b for the input x_k of iteration k -- the
 *     spectral convergence; exactly 0 when the numerator is 0, +inf when only the denominator is.  fp32 partial sums per wave in a fixed
 *     lane order, float64 across bins and blocks in a fixed order, no atomics: bit-identical from run to run, as is the audio.
 * momentum in [0, 1), n_iter >= 1, else TT_E_BADARG.  Scratch: tt_cqt_griffin_lim_scratch_bytes(B * n_blocks, F, sum_len) -- the carve
 * of tt_cqt_scratch_bytes, two audio buffers and the partial sums. */
int64_t tt_cqt_griffin_lim_scratch_bytes(int n_clips, int n_bins, int sum_len);
int tt_cqt_griffin_lim(const tt_cqt_plan* plan, const float* mag, const float* audio_init, float* audio_out, float* conv,
                       void* scratch, int B, int n_blocks, int n_iter, float momentum, int normalize, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Convolution stack. Replaces torch.nn.Conv2d / ConvTranspose2d / ELU as used by
 * timbre_trap/framework/modules.py (ResidualConv2dBlock :721-777, EncoderBlock :597-655,
 * DecoderBlock :658-718, Encoder :396-483, Decoder :486-594) and their autograd backward.
 * ---------------------------------------------------------------------------------------------- */

/* One general direct convolution, used for every layer shape of the model and, with swapped
 * weight strides, for every data-gradient:
 *   y[b,co,ho,t] = act( bias[co] + sum_{ci,kh,kw} w[co*ws_co + ci*ws_ci + kh*ws_kh + kw*ws_kw]
 *                                               * x[b,ci,hi,ti] ) + (res ? res[b,co,ho,t] : 0)
 *   ti = t + kw*dil_w - pad_w
 *   transposed == 0 :  hi = ho*stride_h + kh*dil_h - pad_h
 *   transposed == 1 :  hi = (ho + pad_h - kh*dil_h) / stride_h   when divisible (else no term)
 * bias and res may be NULL.  Weight strides are signed (a flipped kernel = negative stride with
 * `w` pointing at the last tap).
 * res is added AFTER the activation, on every kernel behind this entry point (the model itself never passes one; the parity tests do).
 * Alignment (all fp32 entry points of this section -- tt_conv2d, tt_conv2d_wgrad, tt_resblock_*, tt_sconv_*, tt_tconv_*,
 * tt_channel_sum*): every pointer, scratch included, needs the 4-byte alignment of a float and nothing more.  The faster staging paths
 * (LDS-DMA, 16-byte stores) are chosen per call where T % 4 == 0 and the pointers they touch are 16-byte aligned; any other call takes
 * the register-staged kernels and returns the same results within rounding.  No call is refused for alignment.
 * tests/test_gpu_conv_parity.py holds every element of these entry points to a derived rounding bound against float64, with each
 * pointer in turn one float off a 16-byte boundary, planes down to 1 x 1, and NaN guard bands around every operand. */
int tt_conv2d(const float* x, const float* w, const float* bias, const float* res, float* y,
              int B, int Cin, int Hin, int T, int Cout, int Hout,
              int KH, int KW, int stride_h, int dil_h, int dil_w, int pad_h, int pad_w,
              int transposed, int64_t ws_co, int64_t ws_ci, int64_t ws_kh, int64_t ws_kw,
              int act, void* stream);

/* Weight + bias gradient of the same general convolution (transposed == 0 form):
 *   dw[co*ws_co + ci*ws_ci + kh*ws_kh + kw*ws_kw] += sum_{b,ho,t} g[b,co,ho,t] * x[b,ci,hi,ti]
 *   dbias[co] += sum g[b,co,:,:]          (dbias may be NULL)
 * Accumulates (+=) into dw/dbias: zero them first for a plain gradient.  (Partial sums meet in atomics: the low bits depend on the
 * order of arrival once more than two workgroups add to an element.) */
int tt_conv2d_wgrad(const float* x, const float* g, float* dw, float* dbias,
                    int B, int Cin, int Hin, int T, int Cout, int Hout,
                    int KH, int KW, int stride_h, int dil_h, int dil_w, int pad_h, int pad_w,
                    int64_t ws_co, int64_t ws_ci, int64_t ws_kh, int64_t ws_kw, void* stream);

/* g = dy * ELU'(a) expressed through the saved OUTPUT y = ELU(a):  ELU' = y > 0 ? 1 : y + 1. */
int tt_elu_bwd(const float* dy, const float* y, float* g, int64_t n, void* stream);
/* The same for any TT_ACT_* of tt_conv2d (version 8): g = dy * act'(a) through y = act(a); relu: dy where y > 0, else 0 (torch's
 * threshold_backward); sigmoid: (dy (1 - y)) y.  dy, y, g 16-byte aligned. */
int tt_act_bwd(const float* dy, const float* y, float* g, int64_t n, int act, void* stream);

/* Fused ResidualConv2dBlock forward (modules.py:755-777):
 *   y = ELU(W2 . ELU(W1 (*)_dil x + b1) + b2) + x      x,y: (B,C,H,T), W1 (C,C,3,3), W2 (C,C,1,1)
 * Supported C: 4,8,16,32; dilation 1..3 (other widths: compose tt_conv2d calls).
 * If h1 != NULL the hidden activation ELU(W1 (*) x + b1) (B,C,H,T) is also written, for tt_resblock_bwd; y is the same within
 * rounding either way (not bit for bit: some kernels are chosen by the alignment of h1).  Planes smaller than the halo (H, T < dilation)
 * are valid: taps outside the image contribute nothing. */
int64_t tt_wgrad_scratch_floats(void);

int tt_resblock_fwd(const float* x, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* y, float* h1, int B, int C, int H, int T, int dilation,
                    int flags, void* stream);

/* Fused ResidualConv2dBlock backward.  h1 = the hidden activation saved by tt_resblock_fwd, or NULL to
 * recompute it from x (one more 3x3 convolution, half the saved-activation memory):
 *   inputs  x, h1, dy        outputs  dx (written), dw1/db1/dw2/db2 (accumulated, +=)
 * `ws` is scratch of B*C*H*T + tt_wgrad_scratch_floats() floats (dL/d(conv1 pre-activation), then the
 * per-workgroup partial weight gradients that a second launch sums without atomics); nothing beyond that size is touched.
 * dx must not be NULL (TT_E_BADARG); what dx held is never read. */
int tt_resblock_bwd(const float* x, const float* h1, const float* dy, const float* w1, const float* b1,
                    const float* w2, const float* b2, float* dx, float* dw1, float* db1,
                    float* dw2, float* db2, float* ws, int B, int C, int H, int T, int dilation,
                    int flags, void* stream);

/* bf16-STORAGE residual blocks (C = 4, 8, 16, 32), the "bf16 MFMA conv path" of BASELINE config[2]:
 * activations of a level are bf16, channel-innermost [B][H][T][C] in HBM; weights and their gradients stay fp32 (rounded to
 * bf16 into registers), products accumulate in fp32 (v_mfma_f32_16x16x32_bf16).  Replaces the three ResidualConv2dBlocks of
 * one EncoderBlock / DecoderBlock (modules.py:621-624, 690-693) when ops.WIDE_STORAGE == 'bf16':
 *   tt_wide_pack    x (B,C,H,T) fp32 planar -> out bf16 [B][H][T][C]          tt_wide_unpack   the inverse   (C = 4..64)
 *   tt_wide_rb_fwd  y = ELU(W2 . ELU(W1 (*)_dil x + b1) + b2) + x ; h1 (may be NULL) = ELU(W1 (*) x + b1) saved for backward
 *   tt_wide_rb_bwd  from x, h1, dy: dx (written), dw1 / db1 / dw2 / db2 (fp32, accumulated +=); ws = tt_wide_scratch_bytes
 *                   bytes of scratch (C = 32: dL/d(conv1 pre-activation) in bf16, then per-workgroup partial gradients; C = 4, 8, 16
 *                   keep that tensor in LDS and need the partial gradients only -- C = 16: tt_wide_onepass_scratch_bytes).
 * Alignment and smallest planes of the cl16 entry points, as far as tests/test_gpu_cl16_parity.py holds them (element-wise float64
 * parity through this ABI in both element types, guard bands of NaN and of a large finite value around every operand, planes down
 * to one pixel).  A cl16 pointer that misses its requirement is refused with TT_E_BADARG before anything is launched:
 *   tt_wide_pack / tt_wide_unpack   the cl16 side (out / in) 16-byte aligned; the fp32 planar side 4 bytes.  Any H, T > 0 (T even at C = 4).
 *   tt_gate16, tt_skip_join16_*, tt_scaled_add16, tt_dot16   every 16-bit pointer 16-byte aligned; s, ds, out (fp32) 4 bytes.
 *   tt_convin16[_1]_*, tt_convout16[_1]_*   cl16 tensors 8-byte aligned (one pixel of 4 channels; a batch half of an odd plane is no
 *                   more than that); every fp32 operand and ws 4 bytes -- the 16-byte staging of a planar operand is chosen per call
 *                   where T % 4 == 0 AND that operand (x; dy and the saved y of tt_convout16[_1]_bwd) is 16-byte aligned, any other
 *                   call stages by 4-byte loads with the same results within rounding.  Any H, T > 0.
 *   tt_latent16_*   every cl16 pointer (in, gy, g, out) and ws 16-byte aligned (LDS-DMA on g and on the operands prepared in ws);
 *                   z, w, bias, out (fp32), dw, db 4 bytes.  T % 16 == 0, E >= 1, B >= 1, D >= 1.
 *   tt_sconv16_*, tt_tconv16_*   every cl16 pointer (x, y, dy / g, dx) 16-byte aligned (LDS-DMA on the un-gated operand of the weight
 *                   gradient, both operands in the pregated forms; 16-byte pieces elsewhere); w, b, dw, db and ws (fp32 partials)
 *                   4 bytes.  tt_sconv16_*: H >= 4 (TT_E_BADARG below), any T > 0 (even at C = 4); tt_tconv16_*: any H, T > 0.
 *   tt_wide_rb_fwd[_join], tt_wide_rb_bwd, _bwd_onepass, _bwd_fused, tt_wide_level_bwd[_gated[_join]]   every cl16 pointer (x, y, h1,
 *                   skip, dy, dx, tmp0, tmp1, skip_g, each x[i] / h1[i] of a level) and ws 16-byte aligned (LDS-DMA on x, h1, dy and
 *                   on the dA1 region of ws; 16-byte pieces elsewhere); the level call tests all of them before its first launch.
 *                   w1, b1, w2, b2, skip weights and the fp32 gradients 4 bytes.  Any H, T > 0 (T even at C = 4): planes smaller than
 *                   the halo are valid, taps outside the image contribute nothing -- read from the index arithmetic of every kernel
 *                   behind these entry points (the test file's docstring, per kernel) and run down to (1, 2) (block) and (3, 6)
 *                   (level).  ws at C = 4, 8, 16 holds fp32 partials only; the 16 bytes are asked at every width all the same.
 * The level calls are held there as the claims below state them: tt_wide_level_bwd bit-identical to block-by-block calls, the gated
 * forms against the plain call. */
int64_t tt_wide_scratch_bytes(int B, int C, int H, int T);
int tt_wide_pack(const float* x, void* out, int B, int C, int H, int T, void* stream);
int tt_wide_unpack(const void* in, float* y, int B, int C, int H, int T, void* stream);
int tt_wide_rb_fwd(const void* x, const float* w1, const float* b1, const float* w2, const float* b2, void* y, void* h1,
                   int B, int C, int H, int T, int dilation, void* stream);
/* The same block with a weighted skip join in its epilogue (round 6): y = block(x) + skip_weights[skip_idx] * skip[b mod skip_B] --
 * the join behind a DecoderBlock (reference modules.py:112 `skip_weights[i] * embedding`, :569-589 `y = y + skip`) without a pass of
 * its own: skip = an encoder embedding of skip_B clips, same C / H / T and element type (B % skip_B == 0; B = 2 skip_B when the decoder
 * runs the reconstruction and the transcription decode as one batch).  skip_weights may be NULL (scale 1).  One rounding of the joined
 * value.  Backward: the block's own backward on the incoming gradient (tt_wide_rb_bwd / tt_wide_level_bwd) + tt_skip_join16_bwd. */
int tt_wide_rb_fwd_join(const void* x, const float* w1, const float* b1, const float* w2, const float* b2, void* y, void* h1,
                        const void* skip, const float* skip_weights, int skip_idx, int skip_B, int B, int C, int H, int T, int dilation,
                        void* stream);
int tt_wide_rb_bwd(const void* x, const void* h1, const void* dy, const float* w1, const float* w2, const float* b2,
                   void* dx, float* dw1, float* db1, float* dw2, float* db2, void* ws, int B, int C, int H, int T,
                   int dilation, void* stream);
/* The backward of ALL residual blocks of one level in one call (modules.py:621-624 / 690-693 differentiated: block nblocks-1 first):
 * tt_wide_rb_bwd for every block -- x[i], h1[i], w1[i], w2[i], b2[i], dilations[i]; dy enters the last block, dx leaves the first,
 * tmp0 / tmp1 (nblocks > 1) are two (B,C,H,T) 16-bit buffers for the gradients between the blocks -- with the partial-sum reduces
 * of all blocks DEFERRED into one launch at the end (two launches fewer per level; same sums in the same order, so every output is
 * bit-identical to nblocks calls of tt_wide_rb_bwd).  ws = tt_wide_level_scratch_bytes(nblocks, B, C, H, T) bytes; nblocks <= 4. */
int64_t tt_wide_level_scratch_bytes(int nblocks, int B, int C, int H, int T);
int tt_wide_level_bwd(int nblocks, const void* const* x, const void* const* h1, const void* dy, const float* const* w1,
                      const float* const* w2, const float* const* b2, void* dx, void* tmp0, void* tmp1, float* const* dw1,
                      float* const* db1, float* const* dw2, float* const* db2, void* ws, int B, int C, int H, int T,
                      const int* dilations, void* stream);
/* The same with the gradient leaving the level ALREADY GATED for the layer in front of it: dx = (d loss / d x[0]) * ELU'(x[0]).  In the
 * reference every residual level but the encoder's first sits behind a layer that ends in an ELU (modules.py:626-630 sconv + ELU ->
 * the next EncoderBlock's block1; :683-693 tconv + ELU -> block1), so x[0] IS that layer's saved output and the product is the first
 * thing its backward computes; done here, in the epilogue of the first block's data gradient where x[0] is at hand, that layer's
 * backward (tt_sconv16_bwd_pregated / tt_tconv16_bwd_pregated below) reads one tensor less and stages nothing through registers.
 * All other outputs as tt_wide_level_bwd. */
int tt_wide_level_bwd_gated(int nblocks, const void* const* x, const void* const* h1, const void* dy, const float* const* w1,
                            const float* const* w2, const float* const* b2, void* dx, void* tmp0, void* tmp1, float* const* dw1,
                            float* const* db1, float* const* dw2, float* const* db2, void* ws, int B, int C, int H, int T,
                            const int* dilations, void* stream);
/* tt_wide_level_bwd_gated with the backward of a weighted skip join riding on it (round 6).  x[0], the level's input, is at the same time
 * the encoder embedding e of a skip connection (reference modules.py:112, :569-589: `y + skip_weights[i] * e` in the decoder); skip_g =
 * the gradient that reached that join's output, skip_reps (1 or 2) batches of B clips back to back (2: the pair decode).  The first block's
 * gated epilogue then writes  dx = (dy + W1^T (*) dA1 + skip_weights[skip_idx] * (g[0] + g[1])) * ELU'(x[0])  -- the embedding's two
 * gradient contributions in one tensor, so that nothing is left to add -- and  skip_dw[skip_idx] += <g[0] + g[1], x[0]>  (times 1 / S under
 * tt_set_loss_scale).  Two more loads per lane and pixel instead of tt_skip_join16_bwd's pass over five tensors.  dilations[0] must be 1
 * (TT_E_UNSUPPORTED before anything is launched otherwise).  Returns 0 with the level's backward AND the join done: the first block's
 * kernel has the riding form at every width (C = 4, 8 k_nrb_bwd_fused, C = 16 the strips, C = 32 k_wrb_dxw); never success with the join
 * left out.  (Version 16 removed the positive return code 1, "level done, join not", with the A/B kernel dispatches -- the
 * per-stage narrow kernels, the separate data- and weight-gradient kernels, the forced one-pass choice -- that were its only source.) */
int tt_wide_level_bwd_gated_join(int nblocks, const void* const* x, const void* const* h1, const void* dy, const float* const* w1,
                                 const float* const* w2, const float* const* b2, void* dx, void* tmp0, void* tmp1, float* const* dw1,
                                 float* const* db1, float* const* dw2, float* const* db2, void* ws, int B, int C, int H, int T,
                                 const int* dilations, const void* skip_g, int skip_reps, const float* skip_weights, int skip_idx,
                                 float* skip_dw, void* stream);
/* g *= ELU'(y) in place on n 16-bit elements (n % 8 == 0, both pointers 16-byte aligned; else TT_E_BADARG): the same factor for a gradient that reaches such a layer by another way
 * (a skip connection, a caller's own use of an encoder embedding; ops.GateTapFn). */
int tt_gate16(void* g, const void* y, int64_t n, void* stream);
/* The whole backward of one block in ONE pass from x and dy only (csrc/conv_level_bf16.hip; C = 16, 32, else
 * TT_E_UNSUPPORTED): the hidden activation is recomputed per tile (bit-identical to what tt_wide_rb_fwd would have stored),
 * dL/d(conv1 pre-activation) stays in LDS -- reads x and dy, writes dx.  The forward can then run with h1 = NULL.
 * Same results as tt_wide_rb_bwd (modules.py:755-777 differentiated).  ws = tt_wide_fused_scratch_bytes(C) bytes. */
int64_t tt_wide_fused_scratch_bytes(int C);
int tt_wide_rb_bwd_fused(const void* x, const void* dy, const float* w1, const float* b1, const float* w2, const float* b2,
                         void* dx, float* dw1, float* db1, float* dw2, float* db2, void* ws, int B, int C, int H, int T,
                         int dilation, void* stream);
/* The whole backward of one block in ONE pass from x, the SAVED h1 and dy (csrc/conv_level_bf16.hip k_wrb_bwds; C = 16, 32, else
 * TT_E_UNSUPPORTED): a workgroup walks a strip of 32 columns downwards, the pointwise chain runs once per image row (+ the column
 * halo), dL/d(conv1 pre-activation) lives in a ring of LDS rows only, and the 3x3 weight gradient is indexed by the pixel of x
 * (dW1[tap] = sum_q x[q] (x) dA1[q - tap D]) so that x needs no halo: h1, dy, x in and dx out -- 4 tensors of HBM traffic where
 * tt_wide_rb_bwd's per-stage kernels move 7; nothing is recomputed.  Same results as the per-stage kernels: dx bit-identical, the
 * fp32 weight / bias gradients equal up to summation order (modules.py:755-777 differentiated).
 * ws = tt_wide_onepass_scratch_bytes(C) bytes (<= tt_wide_scratch_bytes).  tt_wide_rb_bwd itself takes this path where
 * tt_wide_rb_bwd_is_onepass(C, dilation) says 1 (measured per width: C = 16). */
int64_t tt_wide_onepass_scratch_bytes(int C);
int tt_wide_rb_bwd_onepass(const void* x, const void* h1, const void* dy, const float* w1, const float* w2, const float* b2,
                           void* dx, float* dw1, float* db1, float* dw2, float* db2, void* ws, int B, int C, int H, int T,
                           int dilation, void* stream);
int tt_wide_rb_bwd_is_onepass(int C, int dilation);
/* What the loaded code object holds for one of the block-backward kernels (version 15; diagnostic, no launch, needs a device):
 * *local_bytes = private (scratch) memory per lane -- stack objects and register spills, 0 for a kernel that keeps everything in
 * registers -- and *num_regs = its vector registers (hipFuncAttributes::localSizeBytes / numRegs).  kernel: TT_BWD_KERNEL_STRIPS
 * (k_wrb_bwds, C = 16 / 32), TT_BWD_KERNEL_DXW (k_wrb_dxw, C = 32; version 16: no longer compiled at C = 16), TT_BWD_KERNEL_NARROW (k_nrb_bwd_fused, C = 4 / 8); dilation
 * 1..3; form 0 = plain, 1 = gated, 2 = riding (a skip join on the gated epilogue) -- the last two exist at dilation 1 only, the riding
 * strips at C = 16 only.  TT_E_UNSUPPORTED for a combination that is not compiled; > 0: the hipError_t of the attribute query. */
#define TT_BWD_KERNEL_STRIPS 0
#define TT_BWD_KERNEL_DXW    1
#define TT_BWD_KERNEL_NARROW 2
int tt_wide_bwd_kernel_attr(int kernel, int C, int dilation, int form, int* local_bytes, int* num_regs);

/* bf16 channel-innermost (4,1) strided / transposed layers between the levels (csrc/conv_stride_bf16.hip): the bf16-storage
 * counterparts of tt_sconv_* / tt_tconv_* below.  x, y, dy, dx are bf16 [B][H][T][channels]; w (2C, C, 4, 1), b and their
 * gradients fp32.  C = the narrower side's channel count (4, 8, 16, 32).
 *   tt_sconv16_fwd  x (B,H,T,C)  -> y (B,(H-4)/2+1,T,2C) = ELU(conv + b)          (modules.py:626-630)
 *   tt_tconv16_fwd  x (B,H,T,2C) -> y (B,2H+2+out_pad,T,C) = ELU(tconv + b)       (modules.py:685-689)
 *   *_bwd           from x, the saved OUTPUT y and dy: dx (written, may be NULL), dw / db (accumulated, +=); the ELU gate
 *                   dy * ELU'(y) is applied on the fly inside the data- and weight-gradient kernels.
 *                   ws: tt_stride16_scratch_bytes(C) bytes (per-wave partial gradients). */
int64_t tt_stride16_scratch_bytes(int C);
int tt_sconv16_fwd(const void* x, const float* w, const float* b, void* y, int B, int C, int H, int T, void* stream);
int tt_sconv16_bwd(const void* x, const void* y, const void* dy, const float* w, void* dx, float* dw, float* db, void* ws,
                   int B, int C, int H, int T, void* stream);
int tt_tconv16_fwd(const void* x, const float* w, const float* b, void* y, int B, int C, int H, int T, int out_pad,
                   void* stream);
int tt_tconv16_bwd(const void* x, const void* y, const void* dy, const float* w, void* dx, float* dw, float* db, void* ws,
                   int B, int C, int H, int T, int out_pad, void* stream);
/* *_bwd_pregated: the same from x and g = dy * ELU'(y) (what tt_wide_level_bwd_gated / tt_latent16_expand_gated leave): the saved
 * output is not needed.  tt_tconv16_bwd_pregated with gate_dx = 1 (C = 16, 32; else TT_E_UNSUPPORTED) passes the favour on: dx leaves
 * as dx * ELU'(x) for the layer in front of the first DecoderBlock (Decoder.convin + ELU, modules.py:534-537 -> tt_latent16_*_pregated). */
int tt_sconv16_bwd_pregated(const void* x, const void* g, const float* w, void* dx, float* dw, float* db, void* ws, int B, int C,
                            int H, int T, void* stream);
int tt_tconv16_bwd_pregated(const void* x, const void* g, const float* w, void* dx, float* dw, float* db, void* ws, int B, int C,
                            int H, int T, int out_pad, int gate_dx, void* stream);

/* The (31,1) latent heads on bf16 channels-last embeddings (csrc/latent_bf16.hip; modules.py:446 Encoder.convlat and :534
 * Decoder.convin).  w is the (D', CT, E, 1) weight of either layer (index (d CT + c) E + h); (CT, D') = (32, <= 48) or (64, <= 144);
 * T % 16 == 0.  ws: tt_latent16_scratch_bytes bytes.
 *   tt_latent16_contract  out (B,Dout,T) fp32 = [bias +] sum_{c,h} w[d][c][h] in[b,h,t,c] for d < Dout (D, or D - 1 to skip the
 *                         gradient of a constant last channel); in = x (cl16), or, with gy != NULL, in = x * ELU'(gy) on the fly
 *                         (data gradient of convin from dy and the saved output)
 *   tt_latent16_expand    out (B,CT,E,T) cl16 = sum_d w[d][c][h] z[b,d,t], with bias != NULL: ELU(bias[c] + .); z (B,Dz,T) with
 *                         Dz = D, or Dz = D - 1 and channel D - 1 = the constant `fill` (the indicator of TimbreTrap.decode,
 *                         modules.py:139-142, without the concatenated tensor)
 *   tt_latent16_wgrad     dw += sum_{b,t} z[b,d,t] g[b,h,t,c]  (z as above; g cl16; with gy != NULL gated and db (CT) += sum g) */
int64_t tt_latent16_scratch_bytes(int B, int CT, int D, int E, int T);
int tt_latent16_contract(const void* in, const void* gy, const float* w, const float* bias, float* out, void* ws, int B, int CT,
                         int D, int Dout, int E, int T, void* stream);
int tt_latent16_expand(const float* z, int Dz, float fill, const float* w, const float* bias, void* out, void* ws, int B, int CT,
                       int D, int E, int T, void* stream);
/* The backward uses with a neighbouring layer's ELU gate moved across the layer boundary (tt_wide_level_bwd_gated for the idea):
 *   tt_latent16_expand_gated      data gradient of Encoder.convlat leaving as (.) * ELU'(gy), gy = the saved output of the strided layer
 *                                 in front (its backward: tt_sconv16_bwd_pregated)
 *   tt_latent16_contract_pregated, tt_latent16_wgrad_pregated   backward of Decoder.convin from g = dy * ELU'(y), as
 *                                 tt_tconv16_bwd_pregated(gate_dx = 1) leaves it; y is not read.  The bias gradient rides as the weight
 *                                 gradient's row of a constant-1 input row: needs D < 48 (CT = 32) / D < 144 (CT = 64), else
 *                                 TT_E_UNSUPPORTED -- from BOTH entry points (the pair is one backward; the contraction used to run
 *                                 there), with nothing written. */
/* 1 where the two pregated entry points below take a head of CT channels and D input channels (they need a free input row of the weight
 * gradient's tile for the bias gradient), else 0 -- what a caller asks before it promises the gate (ops.LatDec16Fn). */
int tt_latent16_pregated_ok(int CT, int D);
int tt_latent16_expand_gated(const float* z, const float* w, const void* gy, void* out, void* ws, int B, int CT, int D, int E, int T,
                             void* stream);
int tt_latent16_contract_pregated(const void* g, const float* w, float* out, void* ws, int B, int CT, int D, int Dout, int E, int T,
                                  void* stream);
int tt_latent16_wgrad_pregated(const float* z, int Dz, float fill, const void* g, float* dw, float* db, void* ws, int B, int CT, int D,
                               int E, int T, void* stream);
int tt_latent16_wgrad(const float* z, int Dz, float fill, const void* g, const void* gy, float* dw, float* db, void* ws, int B,
                      int CT, int D, int E, int T, void* stream);
/* Decoder.convin over reps (1 or 2) batches of B clips expanded from the SAME latents z (B,Dz,T) -- TimbreTrap.decode_pair: the
 * reconstruction and the transcription differ only in the constant indicator channel, ind0 in batch 0 and ind1 in batch 1 (Dz = D - 1;
 * with Dz = D there is no such channel and ind0 / ind1 are ignored).  Clip b of the reps * B clips of out / g / gy belongs to clip
 * b mod B of z, the convention of tt_skip_join16_fwd's embeddings.  B is the batch of z; ws: tt_latent16_scratch_bytes(reps * B, ...).
 *   tt_latent16_image_bytes     size of zt, the 16-bit image of z that the forward leaves for the backward (16-byte aligned)
 *   tt_latent16_expand_reps     out (reps B,CT,E,T) cl16 = ELU(bias + expansion) as tt_latent16_expand (bias != NULL) makes it of the
 *                               concatenated batch; z is transposed ONCE, into zt (written whole; no indicator in it)
 *   tt_latent16_contract_reps   out (B,Dout,T) fp32 = sum over the reps batches of the contraction of g, gated by gy where gy != NULL, else
 *                               g arrives gated (tt_latent16_contract_pregated's meaning and its refusals): each batch accumulated apart,
 *                               the finished fp32 results added -- the bits of reps calls and an fp32 add
 *   tt_latent16_wgrad_reps      dw += sum over all reps B clips of z x g, db += sum g, from the image zt of tt_latent16_expand_reps (the
 *                               same Dz, ind0, ind1, reps); gy as above.  The indicator row of dw takes ind0 / ind1 times its batch's sum;
 *                               no gradient with respect to the indicator is formed.
 * reps = 1 gives the results of the entry points above bit for bit. */
int64_t tt_latent16_image_bytes(int B, int CT, int D, int T);
int tt_latent16_expand_reps(const float* z, int Dz, float ind0, float ind1, int reps, const float* w, const float* bias, void* out,
                            void* zt, void* ws, int B, int CT, int D, int E, int T, void* stream);
int tt_latent16_contract_reps(const void* g, const void* gy, const float* w, float* out, void* ws, int B, int CT, int D, int Dout, int E,
                              int T, int reps, void* stream);
int tt_latent16_wgrad_reps(const void* zt, int Dz, float ind0, float ind1, int reps, const void* g, const void* gy, float* dw, float* db,
                           void* ws, int B, int CT, int D, int E, int T, void* stream);

/* The 3x3 boundary convolutions where fp32 planar tensors meet the bf16 channels-last interior (csrc/conv_edge_bf16.hip), for
 * C0 = 4 first-level channels (model_complexity 2):
 *   tt_convin16_fwd   Encoder.convin (modules.py:433): x (B,2,H,T) fp32 -> y = ELU(conv3x3 + b) as cl16 (B,4,H,T); w (4,2,3,3)
 *   tt_convin16_bwd   from x, the saved output y and dy (cl16): dw, db (+=), dx (B,2,H,T) fp32 (written; may be NULL); y == NULL: dy is
 *                     already dy * ELU'(y), as tt_wide_level_bwd_gated of the first level leaves it -- the saved output is not read
 *   tt_convout16_fwd  Decoder.convout (modules.py:560): x cl16 (B,4,H,T) -> y (B,2,H,T) fp32 = conv3x3 + b; w (2,4,3,3)
 *   tt_convout16_bwd  from x and dy (B,2,H,T) fp32: dx cl16 (written), dw, db (+=)
 * ws: tt_edge16_scratch_bytes() bytes (per-workgroup partial gradients).  fp32 arithmetic; only the cl16 tensors are bf16. */
int64_t tt_edge16_scratch_bytes(void);
int tt_convin16_fwd(const float* x, const float* w, const float* b, void* y, int B, int H, int T, void* stream);
int tt_convin16_bwd(const float* x, const void* y, const void* dy, const float* w, float* dx, float* dw, float* db, void* ws,
                    int B, int H, int T, void* stream);
int tt_convout16_fwd(const void* x, const float* w, const float* b, float* y, int B, int H, int T, void* stream);
int tt_convout16_bwd(const void* x, const float* dy, const float* w, void* dx, float* dw, float* db, void* ws, int B, int H,
                     int T, void* stream);
/* The same four with ONE planar channel (version 8; the magnitude variants, modules.py:892-1075: Encoder.convin = Conv2d(1, 4, 3) + ELU,
 * Decoder.convout = Conv2d(4, 1, 3) followed by relu (TimbreTrapMag.decode) or sigmoid (TimbreTrapMagDB.decode)):
 *   tt_convin16_1_fwd   x (B,1,H,T) fp32 -> y cl16 (B,4,H,T); w (4,1,3,3)
 *   tt_convin16_1_bwd   as tt_convin16_bwd, dx (B,1,H,T) (may be NULL); y == NULL: dy is already gated
 *   tt_convout16_1_fwd  x cl16 (B,4,H,T) -> y (B,1,H,T) fp32 = act(conv + b), act = TT_ACT_NONE / TT_ACT_RELU / TT_ACT_SIGMOID in the epilogue
 *   tt_convout16_1_bwd  from x, the saved output y (may be NULL for TT_ACT_NONE) and dy (B,1,H,T): dy is gated by act'(y) inside the kernel
 *                       (relu: y > 0; sigmoid: (1 - y) y); dx cl16 (written, x S), dw (1,4,3,3), db (1) (+=)
 * Weight / bias gradients: one partial per workgroup, added in a fixed order (bit-identical from run to run); ws: tt_edge16_scratch_bytes. */
int tt_convin16_1_fwd(const float* x, const float* w, const float* b, void* y, int B, int H, int T, void* stream);
int tt_convin16_1_bwd(const float* x, const void* y, const void* dy, const float* w, float* dx, float* dw, float* db, void* ws, int B,
                      int H, int T, void* stream);
int tt_convout16_1_fwd(const void* x, const float* w, const float* b, float* y, int B, int H, int T, int act, void* stream);
int tt_convout16_1_bwd(const void* x, const float* y, const float* dy, const float* w, void* dx, float* dw, float* db, void* ws, int B,
                       int H, int T, int act, void* stream);

/* EncoderBlock.sconv (modules.py:626-630): y = ELU(Conv2d(C, 2C, (4,1), stride (2,1))(x) + b).
 * x (B,C,H,T) -> y (B,2C,(H-4)/2+1,T); w (2C,C,4,1).  Supported C: 4,8,16,32. */
int tt_sconv_fwd(const float* x, const float* w, const float* b, float* y, int B, int C, int H, int T,
                 void* stream);
/* Its backward from the saved input x and OUTPUT y: dx (written; may be NULL), dw / db (accumulated, +=);
 * `scratch` holds tt_wgrad_scratch_floats() + numel(dy) floats (reduction partials, then dy * ELU'(y)).
 * dx == NULL skips the data gradient only: dw and db are the same as with it.  With an odd H the last input row feeds no output
 * row and its dx row is exactly 0.  H < 4: TT_E_BADARG.  The same holds for tt_tconv_bwd (H >= 1). */
int tt_sconv_bwd(const float* x, const float* y, const float* dy, const float* w, float* dx, float* dw,
                 float* db, float* scratch, int B, int C, int H, int T, void* stream);

/* DecoderBlock.tconv (modules.py:685-689): y = ELU(ConvTranspose2d(2C, C, (4,1), stride (2,1),
 * output_padding (out_pad,0))(x) + b).  x (B,2C,H,T) -> y (B,C,2H+2+out_pad,T); w (2C,C,4,1). */
int tt_tconv_fwd(const float* x, const float* w, const float* b, float* y, int B, int C, int H, int T,
                 int out_pad, void* stream);
int tt_tconv_bwd(const float* x, const float* y, const float* dy, const float* w, float* dx, float* dw,
                 float* db, float* scratch, int B, int C, int H, int T, int out_pad, void* stream);

/* Batched GEMM for the (31,1) latent layers (modules.py:446 and :534):
 *   for each batch b:  C_b (M,N) = alpha * op(A_b) (M,K) . op(B_b) (K,N) + beta * C_b  [+ bias]
 * row-major, leading dimensions lda/ldb/ldc, batch strides sa/sb/sc (0 = shared operand).
 * If reduce_batch != 0 all batches are summed into ONE C (weight gradients).
 * bias_mode: 0 none, 1 bias[m] per row, 2 bias[m / bias_div] (transposed-conv bias per channel).
 * act = TT_ACT_ELU applies ELU after bias. */
int tt_gemm(const float* A, const float* Bm, float* C, const float* bias,
            int M, int N, int K, int transA, int transB, int64_t lda, int64_t ldb, int64_t ldc,
            int batch, int64_t sa, int64_t sb, int64_t sc, int reduce_batch,
            float alpha, float beta, int bias_mode, int bias_div, int act, void* stream);

/* out[c] += sum over (b, inner) of x[b, c, inner]; x viewed as (B, C, inner).  The partial sums meet in atomics (low bits vary from
 * run to run). */
int tt_channel_sum(const float* x, float* out, int B, int C, int64_t inner, void* stream);
/* The same sum in a fixed order, bit-identical from run to run (version 7): ws is device scratch of at least 2 C + 2048 floats,
 * free until the call's stream has run it. */
int tt_channel_sum_ws(const float* x, float* out, int B, int C, int64_t inner, float* ws, void* stream);

/* y = a + s[idx] * b  (skip connections, modules.py:112 and :569-589); s may be NULL (scale 1),
 * a may be NULL (treated as 0). */
int tt_scaled_add(const float* a, const float* b, const float* s, int idx, float* y, int64_t n,
                  void* stream);
/* Windowed overlap-add of the half-overlapping chunks of TimbreTrap.chunked_inference (modules.py:259-263):
 *   out[row][i * M/2 + m] += window[m] * chunks[i - c0][row][m]   for chunks i = c0 .. c1-1, accumulated in ascending i
 * chunks (c1-c0, rows, M), window (M), out (rows, n_frames) with rows = B*2*F; M % 8 == 0, n_frames % 4 == 0.  Calls with
 * consecutive chunk ranges reproduce the reference's sequential accumulation bit for bit. */
int tt_window_ola(const float* chunks, const float* window, float* out, int64_t rows, int M, int c0, int c1,
                  int64_t n_frames, void* stream);
/* out[0] += sum(a * b) : gradient of one skip weight. */
int tt_dot(const float* a, const float* b, float* out, int64_t n, void* stream);
/* The same two for the bf16 channels-last path (skip joins under autocast; BASELINE configs[4] trains with
 * skip_connections=True): a, b, y bf16 arrays of n elements (16-byte aligned), s and out fp32; fp32 arithmetic,
 * round-to-nearest-even stores. */
int tt_scaled_add16(const void* a, const void* b, const float* s, int idx, void* y, int64_t n, void* stream);
int tt_dot16(const void* a, const void* b, float* out, int64_t n, void* stream);
/* The weighted skip join as ONE pass each way (round 6; reference modules.py:112 `skip_weights[i] * embedding` and :569-589
 * `y = y + skip`), 16-bit channels-last tensors, n = elements of ONE embedding (n % 8 == 0, 16-byte aligned pointers):
 *   fwd:  out[r*n + i] = y[r*n + i] + s[idx] * e[i]              r < reps (1 or 2)
 *   bwd:  t = sum_r g[r*n + i];   de[i] = s[idx] * t  (* ELU'(e[i]) if gate & 1);   ds[idx] += sum_i t * e[i]      (dy = g: not written)
 *         gate & 2: de[i] += instead of = -- de already holds the other contribution to the embedding's gradient (the data gradient of
 *         the encoder level behind it), so that no separate add is left
 * reps = 2: the decoder runs the reconstruction and the transcription decode of the same latents as one batch of 2 B clips
 * (TimbreTrap.decode_pair) and both halves take the same encoder embedding -- read once, never duplicated.  gate: e is the output of a
 * strided layer + ELU whose backward takes its gradient already multiplied by ELU'(e) (tt_sconv16_bwd_pregated): this contribution
 * then carries the factor as well (what tt_gate16 did in a pass of its own).  s may be NULL (scale 1), de or ds may be NULL.
 * Loss scale (tt_set_loss_scale): g and de are 16-bit gradients and stay scaled, ds *= 1/S. */
int tt_skip_join16_fwd(const void* y, const void* e, const float* s, int idx, void* out, int64_t n, int reps, void* stream);
int tt_skip_join16_bwd(const void* g, const void* e, const float* s, int idx, void* de, float* ds, int64_t n, int reps, int gate,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Objectives.  Replace timbre_trap/framework/objectives.py and TimbreTrap.to_activations
 * (modules.py:271-289).
 * ---------------------------------------------------------------------------------------------- */

/* loss[0] = sum((a-b)^2) * scale     (compute_reconstruction_loss, objectives.py:11-33, with
 * scale = 1/(B*T)).  `partials` is scratch of >= 1024 doubles. */
int tt_sqdiff_sum(const float* a, const float* b, float* loss, double* partials, int64_t n,
                  float scale, void* stream);
/* da = 2*(a-b)*gscale[0]*scale ; db = -da   (either may be NULL) */
int tt_sqdiff_bwd(const float* a, const float* b, const float* gscale, float scale, float* da,
                  float* db, int64_t n, void* stream);
/* Both consistency terms at once (objectives.py:77-104: two squared errors against the same, non-detached, second operand):
 * da1 = 2 scale g1[0] (a1 - b), da2 = 2 scale g2[0] (a2 - b), db = -(da1 + da2); g1 / g2 device scalars (NULL = 0), da1 / da2 / db may be
 * NULL; all pointers 16-byte aligned. */
int tt_sqdiff2_bwd(const float* a1, const float* a2, const float* b, const float* g1, const float* g2, float scale, float* da1,
                   float* da2, float* db, int64_t n, void* stream);
/* The loss(es) AND the gradient(s) in one pass (round 5): the same sums as tt_sqdiff_sum (bit-identical values), and, where a pointer is
 * given, da = 2 scale (a - b), db = -da [tt_sqdiff2_sum_grad: da1, da2 for the two terms against the same b, db = -(da1 + da2);
 * partials: 2048 doubles] -- the gradient for an incoming scalar of 1.  The backward pass is then tt_sqdiff_rescale /
 * tt_sqdiff2_rescale with the incoming scalar(s) on the device: every workgroup reads them and returns when they are 1 (the loss enters
 * the total as it is, train.py:453-466), otherwise the stored gradients are multiplied in place (tt_sqdiff2_rescale recomputes db from
 * da1, da2, which it therefore needs; a NULL scalar counts as 0).  All tensor pointers 16-byte aligned. */
int tt_sqdiff_sum_grad(const float* a, const float* b, float* loss, double* partials, int64_t n, float scale, float* da, float* db,
                       void* stream);
int tt_sqdiff2_sum_grad(const float* a1, const float* a2, const float* b, float* l1, float* l2, double* partials, int64_t n, float scale,
                        float* da1, float* da2, float* db, void* stream);
int tt_sqdiff_rescale(float* da, float* db, const float* g, int64_t n, void* stream);
int tt_sqdiff2_rescale(float* da1, float* da2, float* db, const float* g1, const float* g2, int64_t n, void* stream);

/* CQT.to_magnitude (cqtwrapper.py:122-141; version 8): x (outer, 2, inner) -> y (outer, inner) = sqrt(re^2 + im^2). */
int tt_magnitude(const float* x, float* y, int64_t outer, int64_t inner, void* stream);
/* CQT.to_decibels (cqtwrapper.py:143-182; version 8), torchaudio AmplitudeToDB('amplitude', top_db=80) per item of dim 0 restated:
 * for each of `items` items of `per_item` elements, d = 20 log10(max(m, 1e-10)), top = max d over the item, d = max(d, top - 80),
 * and with `rescale` d = 1 + (d - top) / 80.  Two launches (the item maxima in a fixed order: bit-identical from run to run);
 * ws: tt_decibels_scratch_bytes(items) bytes of device scratch.  items <= 65535. */
int64_t tt_decibels_scratch_bytes(int64_t items);
int tt_decibels(const float* m, float* out, int64_t items, int64_t per_item, int rescale, float* ws, void* stream);
/* TimbreTrapMag.to_activations (modules.py:994; version 8): act = tanh(c) of n elements, and its backward dc = dact (1 - act^2). */
int tt_activations1_fwd(const float* coeffs, float* act, int64_t n, void* stream);
int tt_activations1_bwd(const float* act, const float* dact, float* dcoeffs, int64_t n, void* stream);

/* act = tanh(sqrt(re^2 + im^2)) for coeffs (B,2,F,T) -> (B,F,T) */
int tt_activations_fwd(const float* coeffs, float* act, int B, int F, int T, void* stream);
int tt_activations_bwd(const float* coeffs, const float* act, const float* dact, float* dcoeffs,
                       int B, int F, int T, void* stream);

/* compute_transcription_loss (objectives.py:36-74). est,tgt: (B,F,T); loss[0] = mean over (B,T)
 * of sum_F w*(est-tgt)^2;  `frame_scale` (B*T floats) receives the per-frame positive scaling
 * for the backward pass; weighted = weight_positive_class. */
int tt_transcription_loss_fwd(const float* est, const float* tgt, float* loss, float* frame_scale,
                              double* partials, int B, int F, int T, int weighted, void* stream);
/* tt_transcription_loss_fwd that also writes dest = the gradient w.r.t. est for an incoming scalar of 1 (round 5; backward is then
 * tt_sqdiff_rescale(dest, NULL, g, B F T): a device-side check of the incoming scalar) */
int tt_transcription_loss_fwd_grad(const float* est, const float* tgt, float* loss, float* frame_scale, double* partials, float* dest,
                                   int B, int F, int T, int weighted, void* stream);
int tt_transcription_loss_bwd(const float* est, const float* tgt, const float* frame_scale,
                              const float* gscale, float* dest, int B, int F, int T, int weighted,
                              void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimiser.  Replaces torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.AdamW.step
 * (experiments/train.py:334, :493-496) over ONE flat fp32 buffer of n parameters.
 * ---------------------------------------------------------------------------------------------- */
/* norm_out[0] = ||grad||_2 ; partials: >= 1024 doubles of scratch */
int tt_l2norm(const float* x, float* norm_out, double* partials, int64_t n, void* stream);
/* clip coefficient c = min(1, max_norm / (norm[0] + 1e-6)) is applied to grad on the fly (and
 * written back when write_clipped != 0, to match clip_grad_norm_'s in-place semantics). */
int tt_adamw_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, const float* norm,
                  int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                  int step, float max_norm, int write_clipped, int32_t* skipped, void* stream);
/* `skipped` (device, may be NULL): overflow guard of the loss-scaled fp16 backward, the part of torch.amp.GradScaler the reference
 * does without (experiments/train.py:415 has autocast but no scaler).  With norm and skipped given, a NON-FINITE norm[0] makes the
 * call a no-op that adds 1 to skipped[0]; the bias corrections use step - skipped[0], the number of updates actually applied. */

/* Static loss scale of the 16-bit backward, per calling thread (default 1; returns the previous value).  While S != 1 the backward
 * entry points of the 16-bit channels-last layers treat every 16-bit activation gradient they are handed as carrying the factor S
 * and every fp32 gradient as unscaled:
 *   tt_convout16_bwd                      dx (16-bit) = S * (...)            -- the gradient ENTERS the 16-bit region; dw, db unscaled
 *   tt_latent16_expand   (bias == NULL)   out (16-bit) = S * (...)           -- likewise (data gradient of Encoder.convlat)
 *   tt_latent16_wgrad    (gy == NULL)     z (fp32 gradient) is scaled by S on its way to 16 bits; dw *= 1/S
 *   tt_latent16_wgrad    (gy != NULL), tt_latent16_contract (gy != NULL), tt_convin16_bwd, tt_wide_rb_bwd*, tt_wide_level_bwd,
 *   tt_sconv16_bwd, tt_tconv16_bwd, tt_dot16, tt_skip_join16_bwd (ds)
 *                                         every fp32 output (dw, db, dz, dx) *= 1/S; 16-bit data gradients stay scaled
 * With S a power of two this is an exact identity in real arithmetic; in fp16 it lifts activation gradients of ~1e-7 (the loss is a
 * mean over B x T frames) out of the subnormal range.  The value is read on the host when a kernel is launched and passed by value:
 * stream-ordered like any argument, and invisible to other threads.  Forward entry points must be called with S = 1
 * (timbre_trap/framework/ops.py sets it only around its backward calls). */
float tt_set_loss_scale(float scale);

/* ------------------------------------------------------------------------------------------------
 * Helpers on either side of the path.
 * ---------------------------------------------------------------------------------------------- */
/* Per-parameter gradient statistics in ONE launch over the flat gradient buffer (replaces the per-layer
 * `values.grad.norm(2).item()` host syncs of timbre_trap/utils/experiments.py:144-256):
 * for segment s = [offsets[2s], offsets[2s+1]) (element indices into x; 2*n_segments entries, any order, gaps allowed):
 * out[2s] = L2 norm, out[2s+1] = max |g|. */
int tt_segment_stats(const float* x, const int64_t* offsets, int n_segments, float* out, void* stream);
/* Peak picking / thresholding of activations (timbre_trap/utils/processing.py:66-124) on the device.
 * x, out: (n_outer, F, T).  mode 0: keep strict local maxima along F, zero elsewhere (filter_non_peaks);
 * mode 1: x >= threshold (threshold); mode 2: peak && x >= threshold.  Rows f >= f_valid read as zero first (the
 * `activations[valid_freqs] = 0` of experiments/evaluate.py:107-112); f_valid <= 0 or >= F disables the mask. */
int tt_peak_pick(const float* x, float* out, int64_t n_outer, int F, int T, double threshold, int mode, int f_valid,
                 void* stream);
/* Frame-level pitch annotations -> activation targets (timbre_trap/datasets/PitchDataset.py:233-307) in float64:
 * ones at (bins[i], frames[i]), i < n; if radius > 0: correlation along F with the 2*radius+1 `weights` (zero padded,
 * SciPy's symmetric order -> bit-identical to gaussian_filter1d), division by the smallest blurred value over the
 * annotated positions, clip to [0, 1].  out, work: F*T doubles each (work unused when radius == 0). */
int tt_target_activations(const int* bins, const int* frames, int n, const double* weights, int radius, int F, int T,
                          double* work, double* out, void* stream);

/* The same targets from note annotations (timbre_trap/datasets/NoteDataset.py:60-91: notes_to_multi_pitch, :93-123, followed by
 * PitchDataset.multi_pitch_to_activations, PitchDataset.py:233-307; version 13): ones on row bins[i] over the frames lo[i] <= t < hi[i]
 * (tt_note_spans' output, clipped to [0, T)) for every note i < L with 0 <= bins[i] < F -- a dropped note carries bin -1 -- then the
 * blur, the division by the smallest blurred value over the painted positions and the clip of tt_target_activations.  Bit-identical to
 * tt_target_activations on the expanded (bin, frame) pair list.  out, work: F*T doubles each (work unused when radius == 0). */
int tt_target_activations_spans(const int* bins, const int* lo, const int* hi, int L, const double* weights, int radius, int F, int T,
                                double* work, double* out, void* stream);

/* ---- signal-distortion ratio (csrc/sdr.hip; version 10) ------------------------------------------------------------------------------
 * Replaces torchmetrics.audio.SignalDistortionRatio as built and called by experiments/evaluate.py:51,122-127
 * (`sdr_module(synth, audio).item()` per track, on the device, right after sliCQ.decode): the filtered SDR of B clips of N fp32
 * samples with L = filter_length lags, in float64, without FFTs and without a host round trip:
 *     r[l] = sum_n t[n] t[n+l],  b[l] = sum_n t[n] p[n+l]   (linear: zeros beyond the clip's end),  0 <= l < L
 *     Toeplitz(r / |t|^2 (+ load_diag on the diagonal)) h = b / (|t| |p|);   coh = b . h;   SDR = 10 log10(coh / (1 - coh))
 * 1 <= L <= 512 and N >= 1, else TT_E_BADARG.  preds, target: (B, N) fp32 contiguous; every sum is taken in a fixed order (no atomics).
 *   tt_sdr_chunk          samples per workgroup of the correlation kernel (the lengths at which its index arithmetic changes)
 *   tt_sdr_scratch_bytes  bytes of `scratch` for tt_sdr_means and tt_sdr_correlate (experiments/evaluate.py:51,122-127)
 *   tt_sdr_means          zero_mean=True (evaluate.py:51,122-127 leaves it False): means_out[B][2] = {mean(preds), mean(target)} per clip
 *   tt_sdr_correlate      (experiments/evaluate.py:51,122-127) rb_out[B][2L+1] = r[0..L), b[0..L), sum p^2 of the raw signals, or of the
 *                         signals minus `means` (tt_sdr_means' output; NULL: none), subtracted as the samples are read
 *   tt_sdr_finish         (experiments/evaluate.py:51,122-127) norms clamped at 1e-6 like the host function, load_diag added to r[0] when
 *                         has_load_diag != 0, Levinson recursion (L - 1 steps whatever the data); coh_out[B], sdr_out[B] float64.
 *                         coh / (1 - coh) <= 0 gives -inf; an all-zero target gives a non-finite value, not an error. */
int     tt_sdr_chunk(void);
int64_t tt_sdr_scratch_bytes(int B, int64_t N, int L);
int tt_sdr_means(const float* preds, const float* target, int B, int64_t N, void* scratch, double* means_out, void* stream);
int tt_sdr_correlate(const float* preds, const float* target, int B, int64_t N, int L, const double* means, void* scratch,
                     double* rb_out, void* stream);
int tt_sdr_finish(const double* rb, int B, int L, double load_diag, int has_load_diag, double* coh_out, double* sdr_out,
                  void* stream);

/* ---- multi-pitch scoring (csrc/mpe.hip; version 11) ----------------------------------------------------------------------------------
 * Replaces, per track, the host leg of experiments/evaluate.py:100-116 -- `to_array(transcription)`, `activations_to_multi_pitch(...,
 * peaks_only=True)` (datasets/PitchDataset.py:309-348) and `mir_eval.multipitch.evaluate` as called from utils/experiments.py:376-378 --
 * by per-frame integer counts computed where the activations are.  x: (F, T) fp32, T contiguous.  Nothing here uses atomics; every
 * offset into x or into a CSR array is 64-bit.
 *   tt_mpe_max_est / tt_mpe_max_ref   capacities of tt_mpe_match: active bins / reference pitches per frame it holds in LDS
 *   tt_mpe_count   (evaluate.py:107-113; PitchDataset.py:309-348) n_est[t] = number of bins of frame t that pass tt_peak_pick's predicate
 *                  of `mode` 1 (x >= threshold) or 2 (strict local maximum along F && x >= threshold), rows f >= f_valid read as zero
 *                  first; bad_out[t] = OR of bin_bad[f] over those bins (bin_bad: F bytes, NULL: none -- the bins whose frequency lies
 *                  outside mir_eval's [20, 5000] Hz, which mir_eval.multipitch.validate, called from experiments.py:376-378, rejects)
 *   tt_mpe_fill    (PitchDataset.py:309-348) est_bins[est_off[t] .. est_off[t + 1]) = those bins in ascending order; est_off[T + 1] is the
 *                  exclusive prefix sum of tt_mpe_count's n_est (formed by the caller); nothing is written at or beyond `capacity`
 *   tt_mpe_match   (experiments.py:376-378: mir_eval.multipitch.evaluate -> resample_multipitch, compute_num_true_positives) for
 *                  reference frame j < n_ref_frames, whose pitches are ref_midi[ref_off[j] .. ref_off[j + 1]) (float64 MIDI numbers) and
 *                  which reads estimate frame est_idx[j] (T, or anything outside [0, T): an empty frame) with pitches
 *                  est_midi[est_bins[..]] (est_midi: F float64):  n_est[j] = pitches in that estimate frame;  tp[j] = size of a maximum
 *                  matching under fabs(r - e) <= window;  tp_chroma[j] = the same on fmod(., 12) values with distance
 *                  d = fmod(|r - e|, 12), min(d, 12 - d) -- all float64, the expressions of the host scorer, so the counts are equal
 *                  to its counts, not close to them.  A frame with more than tt_mpe_max_ref reference pitches or more than
 *                  tt_mpe_max_est estimates gets tp[j] = -1 and nothing else written. */
int tt_mpe_max_est(void);
int tt_mpe_max_ref(void);
int tt_mpe_count(const float* x, int F, int T, double threshold, int mode, int f_valid, const unsigned char* bin_bad, int* n_est,
                 int* bad_out, void* stream);
int tt_mpe_fill(const float* x, int F, int T, double threshold, int mode, int f_valid, const int64_t* est_off, int64_t capacity,
                int* est_bins, void* stream);
int tt_mpe_match(const int* est_idx, int n_ref_frames, int T, const int64_t* est_off, const int* est_bins, const double* est_midi,
                 int F, const int64_t* ref_off, const double* ref_midi, double window, int* tp, int* tp_chroma, int* n_est,
                 void* stream);

/* ---- note annotations to per-frame lists (csrc/notes.hip; version 13) --------------------------------------------------------------
 * Replaces NoteDataset.notes_to_multi_pitch (timbre_trap/datasets/NoteDataset.py:93-123: a Python loop over the L notes with an np.where
 * over all N frames and an np.append per (note, frame) pair), as called per item from NoteDataset.py:81 and per track from
 * experiments/evaluate.py:67-75, by flat arrays the device consumers read: frame ranges per note for tt_target_activations_spans, a CSR of
 * note indices per frame for tt_mpe_match (gathered through a per-note MIDI table by the caller).  Nothing here uses atomics; every
 * offset into the CSR is 64-bit; the results do not depend on the launch geometry.
 *   tt_note_spans   (NoteDataset.py:119) times: N float64, NON-DECREASING (the caller checks); intervals: (L, 2) float64 onset / offset.
 *                   lo[i], hi[i]: the half-open range of frames t with times[t] >= onset && times[t] < offset -- the reference's
 *                   comparisons in float64, by binary search.  Empty (hi <= lo) when offset <= onset, when the note lies wholly before
 *                   or after the grid, and (lo = hi = 0) when a bound is NaN
 *   tt_note_tile_frames / tt_note_chunk   (NoteDataset.py:117-121) frames per workgroup of the two kernels below / notes they test
 *                   against a tile per pass: the sizes at which their index arithmetic changes
 *   tt_note_count   (NoteDataset.py:117-121) count[t] = number of notes i < L with lo[i] <= t < hi[i], t < N
 *   tt_note_fill    (NoteDataset.py:117-121) note_idx[off[t] .. off[t + 1]) = those notes' indices in ASCENDING order -- the order in
 *                   which the reference appends, so the gathered pitches equal its lists element for element; off[N + 1] is the
 *                   exclusive prefix sum of tt_note_count's count (formed by the caller); nothing is written at or beyond `capacity` */
int tt_note_tile_frames(void);
int tt_note_chunk(void);
int tt_note_spans(const double* times, int N, const double* intervals, int L, int* lo, int* hi, void* stream);
int tt_note_count(const int* lo, const int* hi, int L, int N, int* count, void* stream);
int tt_note_fill(const int* lo, const int* hi, int L, int N, const int64_t* off, int64_t capacity, int* note_idx, void* stream);

/* ---- note events from activation maps (csrc/events.hip; version 21) ------------------------------------------------------------------
 * The way back from the block above: a (B, F, T) activation map (TimbreTrap.transcribe's output; fp32, T contiguous) to note events --
 * pitch row, onset frame, end frame, strength -- where the map is.  No reference counterpart: the reference stops at per-frame lists.
 * A bin is active under tt_peak_pick's predicate of `mode` 1 or 2 (threshold, f_valid: as for tt_mpe_count; a NaN never passes).  Bins are
 * grouped into P pitch rows by group_off (P + 1 int32 on the device, ascending, within [0, F]): row p owns the bins
 * [group_off[p], group_off[p + 1]), possibly none; frame t of row p is active (a = 1) when one of its bins is, with value v = the largest
 * x among the row's active bins.  With G = max_gap every maximal run of at most G zeros of a row that has a one on both sides inside
 * [0, T) is filled; the candidate notes are the maximal runs [t0, t1] of the filled row (a = 1 at both ends); a candidate is kept iff
 * t1 - t0 + 1 >= min_frames.  Candidates are numbered in ascending (item, row, onset) order.  Nothing here uses atomics or reads the
 * environment; every offset is 64-bit; the grids are one-dimensional, so B P ceil(T / 64) may be any size; the results do not depend on
 * the launch geometry.  0 <= max_gap <= 63, min_frames >= 1, sizes >= 1, no null pointer: else TT_E_BADARG and nothing is launched.
 *   tt_events_mask    mask[(b P + p) W + w], W = ceil(T / 64): bit i = a[b, p, 64 w + i]; the bits beyond T are zero
 *   tt_events_count   n_on / n_end[(b P + p) W + w] = candidates that start / end (last frame) in word w of the row, from that word and
 *                     its two neighbours IN THE SAME ROW.  Per row the two counts have equal totals and the i-th start belongs with the
 *                     i-th end, so the two exclusive prefix sums over all B P W entries (formed by the caller, int64) index the same slots
 *   tt_events_fill    item / row / onset of candidate on_off[.] + rank, end (t1 + 1, exclusive) of candidate end_off[.] + rank; nothing is
 *                     written at or beyond `capacity`
 *   tt_events_finish  for candidate i < n_notes (the arrays tt_events_fill wrote): n_active[i] = a = 1 frames in [t0, t1]; peak[i] = max of
 *                     v over them (an exact fp32 value of x; +inf allowed); keep[i] = (t1 - t0 + 1 >= min_frames) */
int tt_events_mask(const float* x, int B, int F, int T, double threshold, int mode, int f_valid, const int* group_off, int P,
                   uint64_t* mask, void* stream);
int tt_events_count(const uint64_t* mask, int B, int P, int T, int max_gap, int* n_on, int* n_end, void* stream);
int tt_events_fill(const uint64_t* mask, int B, int P, int T, int max_gap, const int64_t* on_off, const int64_t* end_off, int64_t capacity,
                   int* item, int* row, int* onset, int* end, void* stream);
int tt_events_finish(const float* x, int B, int F, int T, double threshold, int mode, int f_valid, const int* group_off, int P,
                     const uint64_t* mask, const int* item, const int* row, const int* onset, const int* end, int64_t n_notes,
                     int min_frames, int* n_active, float* peak, int* keep, void* stream);

/* ---- pitch contours and pitch bends of note events (csrc/contours.hip; version 24) ----------------------------------------------------
 * What the block above leaves behind: every pitch there is a bin centre or a row's number, while the map is sampled at several bins per
 * semitone so that intonation, vibrato and slides show in it.  Here every frame of a note, or every entry of a per-frame bin list, gets
 * a pitch refined below the bin spacing.  No reference counterpart: the reference stops at per-frame lists of bin centres.  Every result
 * is an integer, an exact fp32 value, or a float64 value formed by a fixed sequence of individually rounded operations (nothing is
 * contracted into a fused multiply-add; the divide is the correctly rounded one), so a restatement in NumPy scalars gives equal results.
 * x, threshold, mode, f_valid, group_off, P: exactly as for tt_events_mask; the predicate is the same one.  m: the F float64 MIDI
 * numbers of the bins (midi_freqs), on the device.
 *   refine(f, t)      b = x[f], a = x[f - 1], c = x[f + 1] at frame t; a neighbour beyond either end or at f >= f_valid reads as 0.f.
 *                     If a, b, c are all finite and b >= a and b >= c, in fp32: num = a - c; den = (a - b) + (c - b);
 *                     delta = den < 0 ? 0.5f * (num / den) : 0.f (a NaN quotient, inf / inf: 0.f), clamped to [-0.5f, 0.5f].  Otherwise
 *                     (a NaN or infinite sample, a plateau, in mode 1 a larger neighbour) delta = 0.f.  In float64:
 *                     pitch = m[f] + (double)delta * step, step = m[f + 1] - m[f] for delta >= 0 and m[f] - m[f - 1] otherwise; where
 *                     that neighbour does not exist, the other side's spacing; 0 at F = 1
 *   tt_contours_notes   note i < n_notes is (item, row, onset, end)[i] as tt_events_fill wrote them, in any order; its end - onset frames
 *                     own the slots [frame_off[i], frame_off[i + 1]) (frame_off: n_notes + 1 int64, the exclusive prefix sum of
 *                     end - onset, formed by the caller).  Per frame t: among the bins of the row that pass the predicate the one with
 *                     the largest x (ties: the lowest bin; +inf allowed) gives bin, value = x[bin], delta, pitch = refine(bin, t) and
 *                     bend = (int32) rint((pitch - row_pitch[row]) * units) in float64, ties to even, clamped to [-2^30, 2^30], 0 for a
 *                     non-finite product; a frame where no bin passes (bridged by max_gap) gives bin = -1, delta = 0, value = 0,
 *                     pitch = NaN, bend = 0.  row_pitch: P float64 (the pitch of every row); units >= 1 bend units per semitone.
 *                     Per note, over the frames with bin >= 0: n_voiced, bend_sum (int64), bend_min, bend_max (both 0 where n_voiced is
 *                     0).  Every index read from item / row / onset / end / frame_off is clamped before it addresses memory; slots
 *                     of a note beyond its clamped frames get the values of a frame where no bin passes
 *   tt_contours_frames  x (F, T); est_off (T + 1 int64) / est_bins: the per-frame lists tt_mpe_fill wrote.  delta[j], pitch[j] =
 *                     refine(est_bins[j], t) for est_off[t] <= j < est_off[t + 1]; nothing is written at or beyond `capacity`
 * Nothing here uses atomics or reads the environment; every offset is 64-bit; the grids are one-dimensional; the results do not depend on
 * the launch geometry.  Sizes >= 1 (capacity >= 0), mode 1 or 2, no null pointer: else TT_E_BADARG and nothing is launched. */
int tt_contours_notes(const float* x, int B, int F, int T, double threshold, int mode, int f_valid, const int* group_off, int P,
                      const double* m, const double* row_pitch, int units, const int* item, const int* row, const int* onset, const int* end,
                      int64_t n_notes, const int64_t* frame_off, int* bin, float* delta, float* value, double* pitch, int* bend,
                      int* n_voiced, int64_t* bend_sum, int* bend_min, int* bend_max, void* stream);
int tt_contours_frames(const float* x, int F, int T, int f_valid, const int64_t* est_off, const int* est_bins, int64_t capacity,
                       const double* m, float* delta, double* pitch, void* stream);

/* ---- exact t-SNE in two dimensions (csrc/tsne.hip; version 25) ------------------------------------------------------------------------
 * Replaces the TSNE(n_components=2, perplexity=5, n_iter=1000).fit_transform of plot_latents (timbre_trap/utils/visualization.py:139-144)
 * as experiments/latents.py:111-131 calls it on the time-averaged latents of the Bach10 stems -- a call the installed scikit-learn (>= 1.7,
 * which removed n_iter) refuses -- for codes that are already on the device, and for the thousands of per-frame codes the host route does
 * not reach.  The algorithm is scikit-learn's method='exact': float64 throughout, two output dimensions, no atomics, no environment
 * switches; every sum runs in an order that depends on N alone, so two runs agree bit for bit and a run split in two equals the whole.
 * 2 <= N <= 16384 (P within 2 GiB), D >= 1, 0 < perplexity < N, no null pointer, every pointer a multiple of 8 bytes: else TT_E_BADARG and
 * nothing is launched.  All pointers are device pointers; the entries neither allocate nor synchronise.
 *   tt_tsne_scratch_bytes  (visualization.py:139-144; latents.py:111-131) bytes of `scratch` for the other two entries; TT_E_BADARG for an N
 *                          out of range
 *   tt_tsne_affinities     (visualization.py:139-144; latents.py:111-131) x (N, D), fp32 (dtype 0) or fp64 (dtype 1), converted to float64.
 *                          d_ij = sum over d ascending of (x_id - x_jd)^2, every operation rounded on its own (not the Gram identity): d_ij
 *                          and d_ji are the same bits and d_ii = 0.  Per row i scikit-learn's search for beta_i such that the entropy of
 *                          p_j ~ exp(-beta_i d_ij), j != i, equals log(perplexity): beta = 1; per evaluation s = sum_j exp(-beta d_ij)
 *                          (1e-8 where that is 0), H = log(s) + beta (sum_j d_ij exp(-beta d_ij)) / s; H > log(perplexity): the lower bound
 *                          becomes beta, and beta doubles (no upper bound yet) or moves to the midpoint; otherwise the mirror image with
 *                          halving.  EXACTLY 128 evaluations, no tolerance exit: a bracket closes to rounding, and beta stays finite
 *                          (2^+-127) where it never brackets.  beta_i (output, N doubles) and s_i are those of the last evaluation.
 *                          C_ij = exp(-beta_i d_ij) / s_i, P_ij = max((C_ij + C_ji) / T, DBL_EPSILON) for i != j and 0 on the diagonal,
 *                          T = max(sum_ij (C_ij + C_ji), DBL_EPSILON) added in a fixed order.  P (output, N x N doubles) is symmetric bit
 *                          for bit; the distances exist only in its buffer
 *   tt_tsne_run            (visualization.py:139-144; latents.py:111-131) iterations it0 .. it1 - 1 (0 <= it0 <= it1) of scikit-learn's
 *                          _gradient_descent on the caller's state Y, U (the update), gains, each N x 2 doubles, in and out; one call
 *                          enqueues all its iterations.  At iteration it: e = exaggeration and m = momentum0 while it < explore_iters, else
 *                          e = 1 and m = momentum1.  w_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} w_ij,
 *                          grad_i = 4 (e sum_j p_ij w_ij (y_i - y_j) - (sum_j w_ij^2 (y_i - y_j)) / Z) -- scikit-learn's
 *                          4 sum_j (e p_ij - q_ij) w_ij (y_i - y_j) without its clamp of q_ij = w_ij / Z at DBL_EPSILON, which needs
 *                          |y_i - y_j| > 1e7 / N to act; gains += 0.2 where U grad < 0, else gains *= 0.8, floored at min_gain;
 *                          U = m U - learning_rate (grad gains); Y += U.  There is NO early stop (it would take a host round trip per
 *                          check): exactly it1 - it0 iterations run.  Afterwards, from the FINAL Y and without exaggeration:
 *                          kl_out[0] = sum_{i != j} p_ij log(max(p_ij, eps) / max(w_ij / Z, eps)), eps = DBL_EPSILON, and gnorm_out[0] = the
 *                          2-norm of grad (e = 1); it0 == it1 computes only these.  exaggeration, learning_rate > 0, momenta in [0, 1),
 *                          min_gain >= 0, explore_iters >= 0 */
int64_t tt_tsne_scratch_bytes(int N);
int tt_tsne_affinities(const void* x, int dtype, int N, int D, double perplexity, double* P, double* beta, void* scratch, void* stream);
int tt_tsne_run(const double* P, int N, double* Y, double* U, double* gains, int it0, int it1, int explore_iters, double exaggeration,
                double learning_rate, double momentum0, double momentum1, double min_gain, double* kl_out, double* gnorm_out, void* scratch,
                void* stream);

/* ---- note-level scoring (csrc/notescore.hip; version 23) -----------------------------------------------------------------------------
 * Precision / recall counts of estimated notes against reference notes, in the manner of mir_eval.transcription.match_notes, from notes
 * that are on the device.  No reference counterpart: the reference has no note-level score.  The rule is the one stated in
 * timbre_trap/utils/metrics/notescore.py (note_counts), evaluated in float64 with its expressions, so the counts equal the host's, not close
 * to them: with rnd(x) = rint(x * 1e4) / 1e4, reference i and estimate k of one item are an ONSET PAIR when
 * rnd(|on_i - on_k|) <= onset_tolerance && |p_i - p_k| <= pitch_tolerance, and also an OFFSET PAIR when
 * rnd(|off_i - off_k|) <= max(offset_ratio * (off_i - on_i), offset_min_tolerance) (a NaN anywhere: not a pair).
 * Both note lists are flat arrays sorted by (item, onset) -- NaN onsets last within an item -- with ref_seg / est_seg (n_items + 1 int64)
 * the bounds of every item's run; items lie in [0, n_items) (a note outside has no partner).  Node v < n_ref is reference v, node
 * n_ref + k is estimate k; n_ref, n_est >= 1 and n_ref + n_est < 2^31.  Nothing here uses atomics or recursion; every index read from an
 * operand is clamped before it becomes an address; the results do not depend on the launch geometry.  A missing pointer or a size out
 * of range: TT_E_BADARG and nothing is launched.
 *   tt_notescore_max     references and estimates per connected component that tt_notescore_match holds (>= 64)
 *   tt_notescore_times   onset[i] = (double)(onset_frame[i] * hop_int) * hop_mul / denom, offset[i] likewise from end_frame[i]: the
 *                        arithmetic of events_to_notes (hop_int = hop_length, hop_mul = 1, denom = sample_rate; or hop_int = 1,
 *                        hop_mul = seconds per frame, denom = 1), 1 <= n < 2^31
 *   tt_notescore_ranges  lo[v], hi[v] (n_ref + n_est int32): the slice of the OTHER list, inside v's item, whose onsets lie within
 *                        onset_tolerance + 1e-4 of v's -- a superset of v's onset pairs
 *   tt_notescore_labels  one round of minimum-label propagation with pointer jumping over the onset pairs: label_out[v] = the smallest of
 *                        label_in over v, its onset pairs and what following label_in from there reaches in six steps.  label_in !=
 *                        label_out, n_ref + n_est int32 each, starting from label[v] = v.  Where label_out[v] != label_in[v]: *changed = 1
 *                        and item_mark[item of v] = mark.  At the fixed point (a round that leaves *changed alone) label[v] is the smallest
 *                        node of v's connected component
 *   tt_notescore_match   label: the fixed point; {ref,est}_label_sorted / {ref,est}_perm: each side's labels in ascending order and the
 *                        note index behind every position.  For reference v with label[v] == v: tp[v] / tp_no_offset[v] = size of a
 *                        maximum matching of the offset-and-onset pairs / of the onset pairs within v's component; 0 for every other
 *                        v < n_ref.  A component with more than tt_notescore_max references or estimates: both 0 and
 *                        item_flag[item of v] = 1 (item_flag: n_items int32, zeroed by the caller)
 *   tt_notescore_sums    out[b][5] int64 = {n_ref, n_est, sum tp, sum tp_no_offset, item_flag[b] != 0} of item b from its two runs */
int tt_notescore_max(void);
int tt_notescore_times(const int* onset_frame, const int* end_frame, int64_t n, int64_t hop_int, double hop_mul, double denom, double* onset,
                       double* offset, void* stream);
int tt_notescore_ranges(const int* ref_item, const double* ref_onset, int64_t n_ref, const int* est_item, const double* est_onset,
                        int64_t n_est, const int64_t* ref_seg, const int64_t* est_seg, int n_items, double onset_tolerance, int* lo, int* hi,
                        void* stream);
int tt_notescore_labels(const int* ref_item, const double* ref_pitch, const double* ref_onset, int64_t n_ref, const int* est_item,
                        const double* est_pitch, const double* est_onset, int64_t n_est, const int* lo, const int* hi,
                        double onset_tolerance, double pitch_tolerance, const int* label_in, int* label_out, int* changed, int* item_mark,
                        int n_items, int mark, void* stream);
int tt_notescore_match(const int* label, const int* ref_label_sorted, const int* ref_perm, const int* est_label_sorted, const int* est_perm,
                       const int* ref_item, const double* ref_pitch, const double* ref_onset, const double* ref_offset, int64_t n_ref,
                       const double* est_pitch, const double* est_onset, const double* est_offset, int64_t n_est, double onset_tolerance,
                       double pitch_tolerance, double offset_ratio, double offset_min_tolerance, int* tp, int* tp_no_offset, int* item_flag,
                       int n_items, void* stream);
int tt_notescore_sums(const int* tp, const int* tp_no_offset, int64_t n_ref, int64_t n_est, const int64_t* ref_seg, const int64_t* est_seg,
                      const int* item_flag, int n_items, int64_t* out, void* stream);

/* ---- frame-level pitch annotations to batched targets (csrc/pitch.hip; version 14) ---------------------------------------------------
 * Replaces, per item of an MPEDataset, PitchDataset.resample_multi_pitch (timbre_trap/datasets/PitchDataset.py:194-231: interp1d over the
 * track's frame times, then a list comprehension over the item's frames) followed by PitchDataset.multi_pitch_to_activations
 * (PitchDataset.py:233-307) and the `.float()` of train.py:394, as PitchDataset.__getitem__ calls them (PitchDataset.py:164-192), for a
 * whole batch in a number of launches that does not depend on the batch, from annotations that stay on the device:
 *     times    float64, the source frame times of every track, concatenated; NON-DECREASING and finite within a track (the caller checks)
 *     tracks   int64 [n_tracks][4] = {base, K, below, above}: track n's K frames are times[base .. base + K) and arena rows base .. base + K;
 *              below / above (in [0, K)) are the frames that stand in for targets before / after the annotated span
 *     row_off  int64, row_off[r] .. row_off[r + 1] are arena row r's values;  bins int32 per value: the nearest bin, -1 for a zero or
 *              out-of-range pitch;  lost uint8 per row: the row holds a non-zero pitch outside the bin range
 * Nothing here uses atomics; offsets into the arena and the output are 64-bit; no result depends on the launch geometry.
 *   tt_pitch_tile_frames / tt_pitch_max_bins / tt_pitch_max_radius   (PitchDataset.py:233-307) frames per workgroup of tt_pitch_targets'
 *                     kernels (the size at which their index arithmetic changes) and the capacities they hold: F <= max_bins,
 *                     radius <= max_radius, else TT_E_BADARG
 *   tt_pitch_scratch_bytes   (PitchDataset.py:233-307) bytes of `scratch` for tt_pitch_targets on B items of T frames
 *   tt_pitch_nearest  (PitchDataset.py:213-229) idx[b][t] = the frame of track track[b] nearest to target[b][t] by the rule of
 *                     interp1d(kind='nearest', assume_sorted=True, bounds_error=False, fill_value=(below, above)): the number of midpoints
 *                     times[i] / 2 + times[i + 1] / 2 (float64, every operation rounded on its own) that are < target, by binary search;
 *                     below for a target < times[0], above for one > times[K - 1] (-inf / +inf padding included); a NaN target sorts
 *                     after every midpoint and fails both comparisons: K - 1.  -1 when track[b] is no track or the track is empty
 *   tt_pitch_targets  (PitchDataset.py:233-307; train.py:394) out[b] (F, T), float64 or (out_float32 != 0) its round-to-nearest-even
 *                     float32 cast: tt_target_activations on the (bin, frame) pairs of item b, whose frame t holds the values of arena
 *                     row tracks[track[b]].base + idx[b][t] (an idx outside [0, K): none), bit for bit -- ones at the bins, then for
 *                     radius > 0 the blur, the division by the smallest blurred value over the item's OWN painted positions, the clip;
 *                     an item without a painted position is all zeros.  flags[b] = OR of lost[] over the rows item b reads (the warning
 *                     of PitchDataset.py:280-283).  B <= 65535. */
int     tt_pitch_tile_frames(void);
int     tt_pitch_max_bins(void);
int     tt_pitch_max_radius(void);
int64_t tt_pitch_scratch_bytes(int B, int T);
int tt_pitch_nearest(const double* times, const int64_t* tracks, int n_tracks, const int* track, const double* target, int B, int T,
                     int* idx, void* stream);
int tt_pitch_targets(const int* idx, const int64_t* tracks, int n_tracks, const int* track, int B, int T, const int64_t* row_off,
                     const int* bins, const unsigned char* lost, const double* weights, int radius, int F, int out_float32, void* scratch,
                     void* out, int* flags, void* stream);

/* ---- random stem mixtures for training batches (csrc/mix.hip; version 18) -------------------------------------------------------------
 * Replaces, per item of a StemMixingDataset (timbre_trap/datasets/BaseDataset.py:272-332), the device-shaped work behind its random
 * draws: the excerpt cut of every stem (AudioDataset.slice_audio, AudioDataset.py:113-141), the sums of the stems' audio
 * (BaseDataset.py:307-320) and the sum and clamp of the annotated stems' target maps (BaseDataset.py:323), for a whole batch in one
 * launch each, from audio that stays on the device:
 *     arena    fp32, the samples of every track, concatenated
 *     tracks   int64 [n_tracks][2] = {base, length}: track n's samples are arena[base .. base + length)
 * All pointers are device pointers.  Nothing here uses atomics, scratch or a work buffer; offsets are 64-bit; every output element is
 * one chain of additions in stem order, so no result depends on the launch geometry and two runs agree bit for bit.  The order is that
 * of an explicit loop over the stems from +0, which is what torch.sum(dim=0) on the CPU gives for up to 4 stems, and for 5 outside the
 * last few elements of a row (tests/test_mix_restatement.py); the sign of a zero is not part of the contract.
 *   tt_mix_tile          (AudioDataset.py:113-141) output samples per workgroup of tt_mix_audio: the N at which its index arithmetic
 *                        changes
 *   tt_mix_targets_tile  (BaseDataset.py:323) output elements of one item's F T that one workgroup of tt_mix_targets covers
 *   tt_mix_audio    (AudioDataset.py:113-141; BaseDataset.py:307-320) y (B, N).  Item b's stems are item_off[b] .. item_off[b + 1]
 *                   (item_off: B + 1 ints, non-decreasing from 0); the first item_split[b] of them are its audio-only group, the rest
 *                   its annotated group (the order separate_ground_truth leaves, utils/data.py:183-195).  Sample i of stem s is
 *                   arena[base + stem_start[s] + i] of track stem_track[s] where 0 <= stem_start[s] + i < length and +0 elsewhere:
 *                   stem_start >= 0 is slice_audio's slice (AudioDataset.py:113-125), stem_start = -pad_left its zero padding
 *                   (:126-141).  y[b] = (sum of the audio-only group) + (sum of the annotated group), each added in fp32 in stem
 *                   order (BaseDataset.py:309, 313, 320); an item without stems is zeros; one stem per item is an excerpt batch.
 *                   Track ids are the caller's to check on the host, where the tables are made (utils/mixing.py raises IndexError):
 *                   the entry sees device pointers only, and a stem whose id is outside [0, n_tracks) reads as silence.
 *                   TT_E_BADARG for a negative size or a missing pointer
 *   tt_mix_targets  (BaseDataset.py:323; train.py:394) maps float64 (S, F, T), the annotated stems' targets in stem order; item_off
 *                   B + 1 ints into them.  out[b] (F, T) = clamp(maps[item_off[b]] + maps[item_off[b] + 1] + ..., 0, 1), added in
 *                   float64 in stem order, as float64 or (out_float32 != 0) rounded once to float32; a NaN stays a NaN as in
 *                   torch.clamp; an item without a map is zeros (maps may be NULL when there is none at all).  Any F, T >= 0 */
int tt_mix_tile(void);
int tt_mix_targets_tile(void);
int tt_mix_audio(const float* arena, const int64_t* tracks, int n_tracks, const int* stem_track, const int64_t* stem_start,
                 const int* item_off, const int* item_split, int B, int64_t N, float* y, void* stream);
int tt_mix_targets(const double* maps, const int* item_off, int B, int F, int64_t T, int out_float32, void* out, void* stream);

/* ---- the FiLM layer of TimbreTrapFiLM (csrc/film.hip; version 17) ---------------------------------------------------------------------
 * Replaces FiLM.forward (timbre_trap/framework/modules.py:847-889: `y = x * self.gamma(condition) + self.beta(condition)` between two
 * transposes) as TimbreTrapFiLM.decode calls it (modules.py:814-844) and its autograd backward, for latents x (B, D, T) fp32 with T
 * contiguous, gamma / beta = nn.Linear(2, D) (gw, bw: (D, 2); gb, bb: (D)) and R = 1 or 2 conditions c_r = (c_r0, c_r1) given in HOST
 * memory (cond, R x 2 floats, read at launch and passed to the kernels by value):
 *     G_r[d] = fl(fl(fl(gw[d][0] c_r0) + fl(gw[d][1] c_r1)) + gb[d]),   Bt_r[d] the same from bw, bb   (for a one-hot condition: the
 *     bits of nn.Linear)
 * Every product and every sum is rounded on its own, nothing is contracted into a fused multiply-add: the reference's bits.  Any
 * B, D, T >= 1; element offsets are 64-bit; rows are read 16 bytes at a time where T % 4 == 0 and the tensors are 16-byte aligned and
 * element by element otherwise, with the same results bit for bit.  No atomics: results are bit-reproducible.  The launch functions
 * neither allocate nor synchronise.
 *   tt_film_tile_frames    (modules.py:883) frames of one (clip, channel) row that one workgroup covers: the T at which the kernels'
 *                          index arithmetic changes
 *   tt_film_scratch_bytes  (modules.py:883) bytes of `ws` for tt_film_bwd with parameter gradients
 *   tt_film_fwd            (modules.py:880-887) y[r B + b][d][t] = fl(fl(x[b][d][t] G_r[d]) + Bt_r[d]); y: (R B, D, T).  R = 2 is the
 *                          pair form (reconstruction and transcription of the same latents): one read of x, two halves written
 *   tt_film_bwd            (autograd of modules.py:883) dy: (R B, D, T).  dx (B, D, T), written unless NULL: fl(G_0 dy_0), for R = 2
 *                          fl(fl(G_0 dy_0) + fl(G_1 dy_1)) -- autograd's sum of the two branches.  dgw, dgb, dbw, dbb: all four or all
 *                          NULL; ACCUMULATED (+=) from P_r[d] = sum_{b,t} x dy_r and S_r[d] = sum_{b,t} dy_r:
 *                              dgw[d][j] += sum_r c_rj P_r,  dgb[d] += sum_r P_r,  dbw[d][j] += sum_r c_rj S_r,  dbb[d] += sum_r S_r
 *                          P_r and S_r: per workgroup at most four fp32 terms in a row, then pairwise; the workgroups' partial sums go
 *                          through ws and a second launch adds them in float64 in a fixed order.  x and ws may be NULL without
 *                          parameter gradients. */
int     tt_film_tile_frames(void);
int64_t tt_film_scratch_bytes(int B, int D, int T, int R);
int tt_film_fwd(const float* x, const float* gw, const float* gb, const float* bw, const float* bb, const float* cond, float* y,
                int B, int D, int T, int R, void* stream);
int tt_film_bwd(const float* x, const float* dy, const float* gw, const float* gb, const float* cond, float* dx, float* dgw, float* dgb,
                float* dbw, float* dbb, void* ws, int B, int D, int T, int R, void* stream);

/* ---- track audio: mono mix, sample-rate conversion, inf-norm (csrc/resample.hip; version 12) ----------------------------------------
 * Replaces the three lines of AudioDataset.get_audio (timbre_trap/datasets/AudioDataset.py:69-77) that stand between a decoded file
 * and the CQT -- `torch.mean(audio, dim=0, keepdim=True)`, `torchaudio.functional.resample(audio, fs, self.sample_rate)`,
 * `audio /= audio.abs().max()` when that maximum is non-zero -- for B tracks x of C channels and L samples, (B, C, L) fp32:
 *     y[b][q new + p] = sum_{k < K} h[p][k] xz[b][q orig + k - width],   K = 2 width + orig,   0 <= p < new,
 * xz = the mono mix (channels added in index order in fp32, then one IEEE divide by C) read as zero outside [0, L); the first
 * Lout = ceil(new L / orig) outputs are kept: conv1d(pad(x, (width, width + orig)), h, stride = orig) transposed and flattened, the
 * arithmetic of torchaudio's sinc resampler.  orig, new: the two rates divided by their gcd.  Every output is one chain of K fused
 * multiply-adds in ascending k; nothing here uses atomics, results are bit-reproducible.
 *   tt_resample_tile         (AudioDataset.py:73) frames q per workgroup of the general kernel: the lengths tile orig at which its
 *                            index arithmetic changes
 *   tt_resample_direct_tile  (AudioDataset.py:73) the same for the kernel that serves new <= 4 with orig <= 8 (2:1, 1:2, 3:2), which
 *                            has one thread per output and does not pay for the general kernel's phase walk
 *   tt_resample_max_taps / tt_resample_max_phases   (AudioDataset.py:73) capacities: K <= max_taps, new <= max_phases; beyond them
 *                            tt_resample and tt_resample_partials return TT_E_BADARG
 *   tt_resample_partials     (AudioDataset.py:76-77) peak slots per clip that tt_resample fills for a track of L samples (= its workgroups
 *                            per clip), or TT_E_BADARG
 *   tt_resample              (AudioDataset.py:70-73) taps_t: the tap table TRANSPOSED, fp32 [K][new] (a wavefront runs along the
 *                            phases and reads a row coalesced); y: (B, Lout), Lout as above or TT_E_BADARG.  peak_partials non-NULL:
 *                            (B, tt_resample_partials(L, orig, new)) floats, every workgroup stores the maximum of |y| over the
 *                            outputs it wrote into a slot of its own; a NaN output makes the slot NaN (torch's max, not fmaxf)
 *   tt_resample_normalize    (AudioDataset.py:75-77) per clip: peak = maximum of its n_partials_per_clip slots (NaN wins);
 *                            y /= peak with an IEEE divide unless peak == 0 (a NaN peak is non-zero, as in Python's `if tensor:`) */
int     tt_resample_tile(void);
int     tt_resample_direct_tile(void);
int     tt_resample_max_taps(void);
int     tt_resample_max_phases(void);
int64_t tt_resample_partials(int64_t L, int orig, int nnew);
int tt_resample(const float* x, int B, int C, int64_t L, const float* taps_t, int orig, int nnew, int width, float* y, int64_t Lout,
                float* peak_partials, void* stream);
int tt_resample_normalize(float* y, int B, int64_t Lout, const float* peak_partials, int64_t n_partials_per_clip, void* stream);

/* ---- fp32-class residual blocks on the 16-bit matrix pipe ("x3": split operands), inference ----------------------------------------
 * csrc/conv_x3.hip.  The three ResidualConv2dBlocks of one wide EncoderBlock / DecoderBlock (modules.py:621-624, 690-693; C = 16, 32,
 * dilation 1..3, else TT_E_BADARG / TT_E_UNSUPPORTED) evaluated to fp32 accuracy without the fp32 matrix instructions: every fp32
 * value v (activations in HBM, weights in LDS) is the pair hi = fp16(v), lo = fp16((v - hi) 2^11) and a product is
 * Whi xhi + 2^-11 (Whi xlo + Wlo xhi) on v_mfma_f32_16x16x32_f16 with fp32 accumulators; bias, ELU, residual add in fp32.  Results agree
 * with the fp32 kernels (tt_resblock_fwd) to a few 1e-7 relative; values beyond fp16's range (|v| > 65504) come out non-finite.
 * tt_x3_rb_fwd / tt_x3_level_fwd save no hidden activation: the no-grad path of ops.residual_level in fp32 mode.  The chain, strided and latent
 * entries below are forward only; the block has a training forward and a backward further down (tt_x3_rb_fwd_train / tt_x3_rb_bwd).
 *   tt_x3_bytes      bytes of one activation tensor in the x3 layout [B][H][T][2][C] halves (= B C H T 4)
 *   tt_x3_pack       x (B,C,H,T) fp32 planar -> x3              tt_x3_unpack   the inverse.  A pair holds v to max(2^-23 |v|, 2^-36):
 *                    2^-23 relative from |v| = 2^-13 upwards, absolute below (derivation: tests/x3_ref.py); the join is exact in fp32
 *   tt_x3_rb_fwd     y = ELU(W2 . ELU(W1 (*)_dil x + b1) + b2) + x; x is an x3 tensor, y an x3 tensor (planar_out = 0; x != y) or an
 *                    fp32 planar (B,C,H,T) tensor (planar_out = 1); weights fp32 (C,C,3,3) / (C,C,1,1)
 *   tt_x3_level_fwd  nblocks blocks (w1[i], b1[i], w2[i], b2[i], dilations[i]); x is fp32 planar (x3_in = 0: packed first) or an x3
 *                    tensor, y fp32 planar (x3_out = 0: written by the last block directly) or an x3 tensor;
 *                    ws = tt_x3_level_scratch_bytes bytes; x3_in with y == x (in place): TT_E_BADARG at every nblocks
 * Alignment (every entry point of csrc/conv_x3.hip, the training, strided and latent ones below included): an x3 / x3n tensor is read by
 * 16-byte LDS-DMA or in 8- / 16-byte pieces and written in 8- / 16-byte pieces, and so is the head of every ws -- each such pointer must be
 * a multiple of 16 bytes, else TT_E_BADARG before anything is launched (the level entries test all of theirs up front):
 *   tt_x3_pack[_scaled] out; tt_x3_unpack[_scaled] in; tt_x3_rb_fwd x, y (x3); tt_x3_rb_fwd_train x, h1, y (x3); tt_x3_rb_bwd x, h1, dy, ws,
 *   dx (x3); tt_x3_level_fwd ws, x (x3_in), y (x3_out); tt_x3n_rb_fwd x (planar_in = 0), y (planar_out = 0); tt_x3n_level_fwd ws;
 *   tt_x3_sconv_fwd / tt_x3_tconv_fwd x (planar_in = 0), y (planar_out = 0); tt_x3_latent_encode x, ws; tt_x3_latent_decode ws, y (x3).
 * fp32 planar tensors, weights, biases, scale, the four gradients and the arguments of tt_x3_grad_scale are reached by 4-byte accesses:
 * any float pointer. */
int64_t tt_x3_bytes(int B, int C, int H, int T);
int64_t tt_x3_level_scratch_bytes(int B, int C, int H, int T);

/* The NARROW levels (C = 4, 8) of the same no-grad fp32 forward with split operands (csrc/conv_x3.hip, k_x3n_conv: lane = pixel,
 * v_mfma_f32_4x4x4_16b_f16; ResidualConv2dBlock, reference modules.py:721-777, as called from TimbreTrap._inference / evaluate.py:94-95).
 * Between the blocks of a level the activations are "x3n" tensors [B][H][T][2][C] halves (hi plane, lo 2^11 plane); the first block
 * reads the fp32 planar (B,C,H,T) tensor of the layer in front (planar_in), the last one stores fp32 planar (planar_out): no pack /
 * unpack passes.  ws: tt_x3n_level_scratch_bytes.  Same value range as tt_x3_*: |v| <= 65504, non-finite beyond. */
int64_t tt_x3n_level_scratch_bytes(int B, int C, int H, int T);
int tt_x3n_rb_fwd(const void* x, int planar_in, const float* w1, const float* b1, const float* w2, const float* b2, void* y,
                  int planar_out, int B, int C, int H, int T, int dilation, void* stream);
int tt_x3n_level_fwd(int nblocks, const float* x, float* y, const float* const* w1, const float* const* b1, const float* const* w2,
                     const float* const* b2, const int* dilations, void* ws, int B, int C, int H, int T, void* stream);
int tt_x3_pack(const float* x, void* out, int B, int C, int H, int T, void* stream);
int tt_x3_unpack(const void* in, float* y, int B, int C, int H, int T, void* stream);
int tt_x3_rb_fwd(const void* x, const float* w1, const float* b1, const float* w2, const float* b2, void* y, int planar_out, int B,
                 int C, int H, int T, int dilation, void* stream);
int tt_x3_level_fwd(int nblocks, const void* x, int x3_in, void* y, int x3_out, const float* const* w1, const float* const* b1,
                    const float* const* w2, const float* const* b2, const int* dilations, void* ws, int B, int C, int H, int T,
                    void* stream);

/* ---- split-operand TRAINING of the wide residual blocks (csrc/conv_x3.hip; opt-in: ops.X3_TRAIN / TTRAP_X3_TRAIN=1) -----------------
 * The forward-with-saved-activations and the backward of one ResidualConv2dBlock (reference modules.py:721-777: forward 755-777, and the
 * autograd backward of those lines that tt_resblock_fwd / tt_resblock_bwd provide on the fp32 matrix instructions) at C = 16, 32,
 * dilation 1..3, on (hi, lo) fp16 pairs: every matrix product -- the two weight gradients, whose K dimension is pixels, included -- is the
 * three-term form on v_mfma_f32_16x16x32_f16 with fp32 accumulators; bias sums, ELU' and the residual add are fp32.  All activation-sized
 * tensors (x, h1, y, dy, dx) are x3 tensors of tt_x3_bytes bytes.
 *   tt_x3_rb_fwd_train  tt_x3_rb_fwd that also stores h1 = ELU(W1 (*)_dil x + b1) as an x3 tensor (x, y, h1 distinct)
 *   tt_x3_grad_scale    scale[0] = S, scale[1] = 1 / S (device memory, no host sync): the power of two that puts abs-max(dy[0..n)) into
 *                       [2^8, 2^9) (exponent clamped to +-120); S = 1 for an all-zero or a non-finite dy.  A pair of halves is exact to
 *                       2^-23 relative only from 2^-13 upwards (2^-36 absolute below), and activation gradients of a mean-reduced loss sit
 *                       at 1e-7 .. 1e-10: every x3 GRADIENT tensor carries S.
 *                       ws: tt_x3_grad_scale_scratch_bytes() bytes
 *   tt_x3_pack_scaled   x3 = split(x * scale[0])            tt_x3_unpack_scaled   y = join(x3) * scale[1]   (scale = NULL: tt_x3_pack / _unpack)
 *   tt_x3_rb_bwd        reads what tt_resblock_bwd reads -- the block input x, h1 and the incoming gradient dy (x3, carrying S):
 *                         g2 = dy ELU'(W2 h1 + b2)      dw2 += sum g2 (x) h1 / S      db2 += sum g2 / S
 *                         g1 = (W2^T g2) ELU'(h1)       db1 += sum g1 / S             dw1[co][ci][tap] += sum g1[co][p] x[ci][p + tap] / S
 *                         dx = dy + W1^T (*)_dil g1     an x3 tensor still carrying S (planar_dx = 0) or fp32 planar (B,C,H,T) times 1 / S
 *                       The weight and bias gradients are summed in a fixed order (per-workgroup partials in ws, then a reduce launch; no
 *                       float atomics): bit-reproducible.  Powers of two are exact, so S never shows in a result.  dx differs from x, h1, dy;
 *                       dx = NULL (the block's input wants no gradient) skips the data-gradient launch;
 *                       ws: tt_x3_rb_bwd_scratch_bytes bytes (g1 as an x3 tensor + the partials).
 * Range: activations or weights beyond +-65504 come out non-finite, never finite and wrong; a non-finite dy gives non-finite gradients.
 * There is no fp32 fallback in training (it would take a host sync per level): the caller's finite check on the loss catches it. */
int tt_x3_rb_fwd_train(const void* x, const float* w1, const float* b1, const float* w2, const float* b2, void* y, int planar_out, void* h1,
                       int B, int C, int H, int T, int dilation, void* stream);
int64_t tt_x3_grad_scale_scratch_bytes(void);
int tt_x3_grad_scale(const float* dy, int64_t n, float* scale, void* ws, void* stream);
int tt_x3_pack_scaled(const float* x, void* out, const float* scale, int B, int C, int H, int T, void* stream);
int tt_x3_unpack_scaled(const void* in, float* y, const float* scale, int B, int C, int H, int T, void* stream);
int64_t tt_x3_rb_bwd_scratch_bytes(int B, int C, int H, int T);
int tt_x3_rb_bwd(const void* x, const void* h1, const void* dy, const float* w1, const float* w2, const float* b2, void* dx, int planar_dx,
                 float* dw1, float* db1, float* dw2, float* db2, const float* scale, void* ws, int B, int C, int H, int T, int dilation,
                 void* stream);
/* The strided layers between and above the wide levels with split operands, so that level -> strided layer -> level never leaves the
 * x3 layout.  x is an x3 tensor (planar_in = 0) or -- the layer that ENTERS the split-operand part of the network -- an fp32 planar
 * (B,C,H,T) tensor (planar_in = 1); y an x3 tensor (planar_out = 0) or fp32 planar (planar_out = 1):
 *   tt_x3_sconv_fwd  EncoderBlock.sconv (modules.py:626-630): y = ELU(Conv2d(C, 2C, (4,1), stride (2,1))(x) + bias); x has C channels and
 *                    H >= 4 rows, y 2C channels and (H - 4) / 2 + 1 rows; C = 16, 32 (x3 input) or C = 8 (planar input)
 *   tt_x3_tconv_fwd  DecoderBlock.tconv (modules.py:683-688): y = ELU(ConvTranspose2d(2C, C, (4,1), stride (2,1),
 *                    output_padding (out_pad, 0))(x) + bias); x has 2C channels and H rows, y C channels and 2H + 2 + out_pad rows;
 *                    C = 16 or 32 (x3 input), C = 32 (planar input)
 * other widths: TT_E_UNSUPPORTED.  Weights fp32 in torch's layouts: (2C, C, 4, 1) for both (the transposed layer's is (in, out, 4, 1)). */
int tt_x3_sconv_fwd(const void* x, int planar_in, const float* w, const float* bias, void* y, int planar_out, int B, int C, int H, int T,
                    void* stream);
int tt_x3_tconv_fwd(const void* x, int planar_in, const float* w, const float* bias, void* y, int planar_out, int B, int C, int H, int T,
                    int out_pad, void* stream);

/* The latent heads with split operands (csrc/conv_x3.hip), (C, D) = (64, 128) or (32, 32), else TT_E_UNSUPPORTED / -1:
 *   tt_x3_latent_encode  Encoder.convlat (modules.py:446) = Conv2d(C, D, (E,1)): x an x3 tensor (B, E, T, 2, C), w (D, C, E, 1), bias (D) or
 *                        NULL, z (B, D, T) fp32
 *   tt_x3_latent_decode  Decoder.convin (modules.py:534) = ELU(ConvTranspose2d(D + 1, C, (E,1))): z (B, Dz, T) fp32 with Dz = D + 1, or
 *                        Dz = D and the last input channel constant = fill; w (D + 1, C, E, 1), bias (C) or NULL; y an x3 tensor
 *                        (B, E, T, 2, C) or fp32 planar (B, C, E, T) (planar_out)
 *   ws = tt_x3_latent_scratch_bytes(C, E, D) bytes (the split weights in operand order, rewritten by every call). */
int64_t tt_x3_latent_scratch_bytes(int C, int E, int D);
int tt_x3_latent_encode(const void* x, const float* w, const float* bias, float* z, void* ws, int B, int C, int E, int D, int T,
                        void* stream);
int tt_x3_latent_decode(const float* z, int Dz, float fill, const float* w, const float* bias, void* y, int planar_out, void* ws, int B,
                        int C, int E, int D, int T, void* stream);

/* ---- fp16 twins ---------------------------------------------------------------------------------------------------------------
 * Every entry point of the 16-bit channels-last path above exists a second time with the suffix _h: the same kernels compiled with
 * fp16 elements (csrc/bf16_common.h, -DTT_F16: v_mfma_f32_*_f16, same layouts, same scratch sizes, same argument meaning; `void*`
 * activation pointers then hold IEEE half instead of bf16).  fp16 is the dtype the reference's own train step runs in
 * (experiments/train.py:415: torch.autocast('cuda') defaults to torch.float16): 11 significant bits per stored activation instead of
 * 8, at the price of fp16's range (normal numbers 6.1e-5 .. 65504; the reference uses no GradScaler, and neither does this path).
 * The Python layer picks the set by the autocast dtype. */
int64_t tt_wide_level_scratch_bytes_h(int nblocks, int B, int C, int H, int T);
int tt_wide_level_bwd_h(int nblocks, const void* const* x, const void* const* h1, const void* dy, const float* const* w1,
                        const float* const* w2, const float* const* b2, void* dx, void* tmp0, void* tmp1, float* const* dw1,
                        float* const* db1, float* const* dw2, float* const* db2, void* ws, int B, int C, int H, int T,
                        const int* dilations, void* stream);
int64_t tt_wide_scratch_bytes_h(int B, int C, int H, int T);
int tt_wide_pack_h(const float* x, void* out, int B, int C, int H, int T, void* stream);
int tt_wide_unpack_h(const void* in, float* y, int B, int C, int H, int T, void* stream);
int tt_wide_rb_fwd_h(const void* x, const float* w1, const float* b1, const float* w2, const float* b2, void* y, void* h1,
                   int B, int C, int H, int T, int dilation, void* stream);
int tt_wide_rb_fwd_join_h(const void* x, const float* w1, const float* b1, const float* w2, const float* b2, void* y, void* h1,
                          const void* skip, const float* skip_weights, int skip_idx, int skip_B, int B, int C, int H, int T, int dilation,
                          void* stream);
int tt_wide_rb_bwd_h(const void* x, const void* h1, const void* dy, const float* w1, const float* w2, const float* b2,
                   void* dx, float* dw1, float* db1, float* dw2, float* db2, void* ws, int B, int C, int H, int T,
                   int dilation, void* stream);
int64_t tt_wide_fused_scratch_bytes_h(int C);
int tt_wide_rb_bwd_fused_h(const void* x, const void* dy, const float* w1, const float* b1, const float* w2, const float* b2,
                         void* dx, float* dw1, float* db1, float* dw2, float* db2, void* ws, int B, int C, int H, int T,
                         int dilation, void* stream);
int64_t tt_wide_onepass_scratch_bytes_h(int C);
int tt_wide_rb_bwd_onepass_h(const void* x, const void* h1, const void* dy, const float* w1, const float* w2, const float* b2,
                           void* dx, float* dw1, float* db1, float* dw2, float* db2, void* ws, int B, int C, int H, int T,
                           int dilation, void* stream);
int tt_wide_rb_bwd_is_onepass_h(int C, int dilation);
int tt_wide_bwd_kernel_attr_h(int kernel, int C, int dilation, int form, int* local_bytes, int* num_regs);
int64_t tt_stride16_scratch_bytes_h(int C);
int tt_sconv16_fwd_h(const void* x, const float* w, const float* b, void* y, int B, int C, int H, int T, void* stream);
int tt_sconv16_bwd_h(const void* x, const void* y, const void* dy, const float* w, void* dx, float* dw, float* db, void* ws,
                   int B, int C, int H, int T, void* stream);
int tt_tconv16_fwd_h(const void* x, const float* w, const float* b, void* y, int B, int C, int H, int T, int out_pad,
                   void* stream);
int tt_sconv16_bwd_pregated_h(const void* x, const void* g, const float* w, void* dx, float* dw, float* db, void* ws, int B, int C,
                              int H, int T, void* stream);
int tt_gate16_h(void* g, const void* y, int64_t n, void* stream);
int tt_tconv16_bwd_pregated_h(const void* x, const void* g, const float* w, void* dx, float* dw, float* db, void* ws, int B, int C,
                              int H, int T, int out_pad, int gate_dx, void* stream);
int tt_latent16_pregated_ok_h(int CT, int D);
int tt_latent16_expand_gated_h(const float* z, const float* w, const void* gy, void* out, void* ws, int B, int CT, int D, int E, int T,
                               void* stream);
int tt_latent16_contract_pregated_h(const void* g, const float* w, float* out, void* ws, int B, int CT, int D, int Dout, int E, int T,
                                    void* stream);
int tt_latent16_wgrad_pregated_h(const float* z, int Dz, float fill, const void* g, float* dw, float* db, void* ws, int B, int CT, int D,
                                 int E, int T, void* stream);
int tt_wide_level_bwd_gated_h(int nblocks, const void* const* x, const void* const* h1, const void* dy, const float* const* w1,
                              const float* const* w2, const float* const* b2, void* dx, void* tmp0, void* tmp1, float* const* dw1,
                              float* const* db1, float* const* dw2, float* const* db2, void* ws, int B, int C, int H, int T,
                              const int* dilations, void* stream);
int tt_wide_level_bwd_gated_join_h(int nblocks, const void* const* x, const void* const* h1, const void* dy, const float* const* w1,
                                   const float* const* w2, const float* const* b2, void* dx, void* tmp0, void* tmp1, float* const* dw1,
                                   float* const* db1, float* const* dw2, float* const* db2, void* ws, int B, int C, int H, int T,
                                   const int* dilations, const void* skip_g, int skip_reps, const float* skip_weights, int skip_idx,
                                   float* skip_dw, void* stream);
int tt_tconv16_bwd_h(const void* x, const void* y, const void* dy, const float* w, void* dx, float* dw, float* db, void* ws,
                   int B, int C, int H, int T, int out_pad, void* stream);
int64_t tt_latent16_scratch_bytes_h(int B, int CT, int D, int E, int T);
int tt_latent16_contract_h(const void* in, const void* gy, const float* w, const float* bias, float* out, void* ws, int B, int CT,
                         int D, int Dout, int E, int T, void* stream);
int tt_latent16_expand_h(const float* z, int Dz, float fill, const float* w, const float* bias, void* out, void* ws, int B, int CT,
                       int D, int E, int T, void* stream);
int tt_latent16_wgrad_h(const float* z, int Dz, float fill, const void* g, const void* gy, float* dw, float* db, void* ws, int B,
                      int CT, int D, int E, int T, void* stream);
int64_t tt_latent16_image_bytes_h(int B, int CT, int D, int T);
int tt_latent16_expand_reps_h(const float* z, int Dz, float ind0, float ind1, int reps, const float* w, const float* bias, void* out,
                            void* zt, void* ws, int B, int CT, int D, int E, int T, void* stream);
int tt_latent16_contract_reps_h(const void* g, const void* gy, const float* w, float* out, void* ws, int B, int CT, int D, int Dout, int E,
                              int T, int reps, void* stream);
int tt_latent16_wgrad_reps_h(const void* zt, int Dz, float ind0, float ind1, int reps, const void* g, const void* gy, float* dw, float* db,
                           void* ws, int B, int CT, int D, int E, int T, void* stream);
int64_t tt_edge16_scratch_bytes_h(void);
int tt_convin16_fwd_h(const float* x, const float* w, const float* b, void* y, int B, int H, int T, void* stream);
int tt_convin16_bwd_h(const float* x, const void* y, const void* dy, const float* w, float* dx, float* dw, float* db, void* ws,
                    int B, int H, int T, void* stream);
int tt_convout16_fwd_h(const void* x, const float* w, const float* b, float* y, int B, int H, int T, void* stream);
int tt_convout16_bwd_h(const void* x, const float* dy, const float* w, void* dx, float* dw, float* db, void* ws, int B, int H,
                     int T, void* stream);
int tt_convin16_1_fwd_h(const float* x, const float* w, const float* b, void* y, int B, int H, int T, void* stream);
int tt_convin16_1_bwd_h(const float* x, const void* y, const void* dy, const float* w, float* dx, float* dw, float* db, void* ws, int B,
                      int H, int T, void* stream);
int tt_convout16_1_fwd_h(const void* x, const float* w, const float* b, float* y, int B, int H, int T, int act, void* stream);
int tt_convout16_1_bwd_h(const void* x, const float* y, const float* dy, const float* w, void* dx, float* dw, float* db, void* ws, int B,
                       int H, int T, int act, void* stream);
int tt_scaled_add16_h(const void* a, const void* b, const float* s, int idx, void* y, int64_t n, void* stream);
int tt_dot16_h(const void* a, const void* b, float* out, int64_t n, void* stream);
int tt_skip_join16_fwd_h(const void* y, const void* e, const float* s, int idx, void* out, int64_t n, int reps, void* stream);
int tt_skip_join16_bwd_h(const void* g, const void* e, const float* s, int idx, void* de, float* ds, int64_t n, int reps, int gate,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTRAP_H */
