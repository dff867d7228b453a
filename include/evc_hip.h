/* evc_hip.h -- C ABI of libevc_hip.so: the MI355X (gfx950) kernels of the decode hot path.
 *
 * Boundary rules: plain pointers and sizes, no torch types, the caller owns every
 * buffer (no allocation inside), every call is stream-ordered on the `stream` argument
 * (a hipStream_t passed as void*), returns 0 on success and a negative EVC_E* code otherwise,
 * never throws.  All tensors are float32.  "NHWC" = [B][H][W][C] contiguous, C fastest.
 *
 * What each entry point replaces in the reference is cited next to it (paths relative to the
 * reference repository root).
 */
#ifndef EVC_HIP_H
#define EVC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define EVC_OK 0
#define EVC_EINVAL (-1)   /* bad shape / null pointer / misaligned channel count */
#define EVC_EUNSUPPORTED (-2)
#define EVC_ELAUNCH (-3)  /* hipGetLastError() != hipSuccess after the launch */

#define EVC_ACT_NONE 0
#define EVC_ACT_SILU 1
#define EVC_ACT_RELU 2

/* How the convolution multiplies (both are fp32 convolutions with fp32 accumulation):
 *   EVC_ARITH_F32     v_mfma_f32_32x32x2_f32: exact fp32 products, k-ordered fmaf chain;
 *   EVC_ARITH_BF16X6  every fp32 operand is split EXACTLY into three bf16 values and the six significant cross
 *                     products run on v_mfma_f32_32x32x16_bf16 (16x the f32 MFMA rate); the dropped terms are below
 *                     one fp32 rounding of a product.  Measured error against fp64 on MI355X: equal to or below
 *                     that of EVC_ARITH_F32 (tools/split_numerics.hip). */
#define EVC_ARITH_F32 0
#define EVC_ARITH_BF16X6 1
/*   EVC_ARITH_F16X3   both operands are scaled by powers of two into fp16's range (weights per tensor at pack time,
 *                     activations by 8 -- nothing is clamped: an element beyond fp16's range comes out as NaN and the
 *                     EVC_RANGE_* word below says beforehand whether one can exist), split 2-way into fp16 (11 + 11 significand bits,
 *                     2^-22 relative) and three cross products run on v_mfma_f32_32x32x16_f16 (bf16 rate); the exact
 *                     inverse scale is applied to the fp32 accumulator.  Half the MFMAs and two thirds of the LDS
 *                     bytes of BF16X6.  Measured error against fp64: BELOW both F32 and BF16X6 for O(1) operands
 *                     (profiles/r02_split_numerics.log) -- fewer accumulator roundings -- but operands spanning more
 *                     than fp16's exponent range are NOT representable: use it only where the input is
 *                     GroupNorm-normalised / activated (the caller's choice, made when packing the weights). */
#define EVC_ARITH_F16X3 2

/* Library / device identification. evc_arch() returns the gfx target the code object was built
 * for ("gfx950"). evc_device_ok() returns 1 when the current HIP device can run it. */
const char* evc_version(void);
const char* evc_arch(void);
int evc_device_ok(void);

/* Measurement aid (bench.py): a one-wave kernel on `stream` that idles for at most spin_us microseconds (<= 10 s), or until
 * the device word *stop (may be NULL) becomes non-zero -- the caller writes it stream-ordered behind the work it wants
 * characterised, so the probe never outlives that work -- and writes out2[0] = shader-clock ticks (s_memtime), out2[1] =
 * 100 MHz reference ticks (s_memrealtime) elapsed meanwhile; out2 is device or pinned host memory.  out2[0] / out2[1] / 10
 * = the shader clock in GHz the chip held while other streams ran -- the convolution kernels run the package into its
 * power cap, so this is what the roofline's clock is. */
int evc_clock_probe(unsigned long long* out2, int spin_us, const unsigned* stop, void* stream);

/* ---- upfirdn2d: the reference's own native op ---------------------------------------------
 * Replaces pybind `upfirdn2d(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0,
 * pad_y1)` (models/better/op/upfirdn2d.cpp:12-23, upfirdn2d_kernel.cu:209-243).  `input` is the
 * reference's (major = N*C, in_h, in_w, minor = 1) view, i.e. NCHW planes; `out` must hold
 * major*out_h*out_w floats with out_h = (in_h*up_y + pad_y0 + pad_y1 - kh)/down_y + 1 (same for w).
 * The FIR kernel (kh*kw <= 64 taps) is a HOST pointer (it is 16 floats in this workload). */
int evc_upfirdn2d_f32(const float* input, float* out, const float* kernel_host, int major, int in_h, int in_w,
                      int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1,
                      int pad_y0, int pad_y1, void* stream);

/* Same maths on an NHWC tensor, with an optional per-(b,c) affine + activation applied to every
 * input sample before filtering (zero padding stays zero).  Fuses get_act_norm + upsample_2d /
 * downsample_2d of ResnetBlockBigGANppGN.forward (models/better/layerspp.py:596-611). */
int evc_upfirdn2d_nhwc_f32(const float* x, float* out, const float* kernel_host, int B, int H, int W, int C,
                           int kh, int kw, int up, int down, int pad0, int pad1, const float* coef_a,
                           const float* coef_s, int act, void* stream);

/* ---- layout -------------------------------------------------------------------------------
 * Pack up to two NCHW tensors (x: C0 planes, cond: C1 planes) into one zero-padded NHWC tensor with
 * Cpad channels: torch.cat([x, cond], 1) of NCSNpp.forward (models/better/ncsnpp_more.py:256-257). */
int evc_pack_nchw_to_nhwc_f32(const float* x0, int C0, const float* x1, int C1, float* out, int Cpad, int B,
                              int H, int W, void* stream);
/* out[b][c][h][w] = in[b][h][w][c] for c < C; `ld` is the NHWC channel stride of `in`. */
int evc_nhwc_to_nchw_f32(const float* in, int ld, float* out, int B, int C, int H, int W, void* stream);

/* ---- GroupNorm ----------------------------------------------------------------------------
 * Per-channel partial moments of an NHWC tensor: partial[b][s][c] = {sum, sum of squares} over the
 * s-th of `nsplit` pixel ranges.  First half of nn.GroupNorm (models/better/layerspp.py:473-477). */
int evc_chan_stats_f32(const float* x, float* partial, int B, int HW, int C, int nsplit, void* stream);

/* Turn moments into per-(b,c) affine coefficients so that  norm(x) = x*coef_a + coef_s :
 *   mode 0: plain group norm;  mode 1: * gamma + beta (AttnBlockpp.GroupNorm_0, final Norm_0);
 *   mode 2: * (1 + scale) + shift, the AdaGN of get_act_norm.forward
 *           (models/better/layerspp.py:518-549); scale = ss[row[b]*ss_ld + c], shift = ...[C + c].
 * Channels come from up to two tensors (virtual concat, C = C0 + C1); groups may straddle them. */
int evc_gn_coeffs_f32(const float* part0, int nsplit0, int C0, const float* part1, int nsplit1, int C1, int B,
                      int HW, int groups, float eps, int mode, const float* gamma, const float* beta,
                      const float* ss, int ss_ld, const int* row, float* coef_a, float* coef_s, void* stream);

/* Range events of the fp16-split arithmetic (EVC_ARITH_F16X3).  That arithmetic scales its operands by powers of two
 * into fp16's range WITHOUT clamping: an operand element beyond the range becomes inf in the split and NaN in the output
 * (loud, never a silently saturated number), and a NaN / inf input stays non-finite.  That last promise covers every
 * export of this header, not only the fp16-split path: clamps, ReLUs and max pools pass a NaN through, as torch does.
 * Whether an operand can leave fp16's range is decided on O(B*C) numbers by the kernels that see every tensor's moments
 * -- the two functions below -- which OR these bits into the caller's sticky device word `events` (may be NULL; never
 * cleared by a kernel):
 *   EVC_RANGE_NONFINITE    a tensor's moments are not finite: it holds a NaN or an infinity;
 *   EVC_RANGE_F16_OPERAND  for some channel |coef_a| * max|x| + |coef_s| >= 65504 / 8: a GroupNorm-ed (and activated,
 *                          |SiLU(v)| <= |v|) operand element MAY leave fp16's range.  Zero means none can (a sufficient
 *                          condition).  Remedy: EVC_ARITH_BF16X6 for that model (host: EVC_CONV_ARITH=bf16x6), or for
 *                          the consumers of the site that raised it only (the _site_ forms below; host:
 *                          EVC_RANGE_RECOVERY=layer). */
#define EVC_RANGE_NONFINITE 1u
#define EVC_RANGE_F16_OPERAND 2u

/* evc_gn_coeffs_f32 that additionally raises *bound_bits (atomic max; the caller zeroes it first) to the bit pattern of
 * the largest {sum of squares} entry among the moments it read: sqrt of that float bounds every element of the tensor(s),
 * because each element belongs to exactly one entry (the NaN pattern 0x7fc00000 when a moment is not finite: consumers
 * then scale by NaN).  Deterministic (max is order-independent).  bound_bits and events may be NULL. */
int evc_gn_coeffs_bound_f32(const float* part0, int nsplit0, int C0, const float* part1, int nsplit1, int C1, int B,
                            int HW, int groups, float eps, int mode, const float* gamma, const float* beta,
                            const float* ss, int ss_ld, const int* row, float* coef_a, float* coef_s,
                            unsigned* bound_bits, unsigned* events, void* stream);
/* The same bound over n_ranges consecutive channel ranges [c_begin + z*c_count, + c_count) of one moments tensor
 * [B][nsplit][C][2], range z into bound_bits[z] (for tensors that are not followed by a GroupNorm: the q | k | v
 * projection feeding attention has three). */
int evc_moments_bound_f32(const float* part, int nsplit, int C, int c_begin, int c_count, int n_ranges, int B,
                          unsigned* bound_bits, unsigned* events, void* stream);

/* Per-site attribution of the range events.  An event SITE is one of these calls inside a network's forward (the
 * caller numbers them; each guards the fp16-split consumers of the tensor it bounds).  The _site_ forms take the caller's
 * site arena `site_events` (one word per site, zeroed by the caller, never cleared by a kernel) and the call's index
 * `site`, and on exactly the conditions above OR the same EVC_RANGE_* bits into BOTH `events` and site_events[site]
 * (either may be NULL; site_events NULL makes them the plain forms).  The extra atomic sits on the branches that already
 * raise: a clean call does the same work as the plain form.  With `events` NULL and site_events set the call still runs
 * the range test but reports to its site word only (a caller that already moved the site's consumers off the fp16 split
 * keeps the global word for the sites that still matter).
 *   evc_gn_coeffs_site_f32:       evc_gn_coeffs_f32 + the event words (no element bound);
 *   evc_gn_coeffs_bound_site_f32: evc_gn_coeffs_bound_f32 + the site word;
 *   evc_moments_bound_site_f32:   evc_moments_bound_f32 + the site word (EVC_RANGE_NONFINITE only, as the plain form). */
int evc_gn_coeffs_site_f32(const float* part0, int nsplit0, int C0, const float* part1, int nsplit1, int C1, int B,
                           int HW, int groups, float eps, int mode, const float* gamma, const float* beta,
                           const float* ss, int ss_ld, const int* row, float* coef_a, float* coef_s, unsigned* events,
                           unsigned* site_events, int site, void* stream);
int evc_gn_coeffs_bound_site_f32(const float* part0, int nsplit0, int C0, const float* part1, int nsplit1, int C1, int B,
                                 int HW, int groups, float eps, int mode, const float* gamma, const float* beta,
                                 const float* ss, int ss_ld, const int* row, float* coef_a, float* coef_s,
                                 unsigned* bound_bits, unsigned* events, unsigned* site_events, int site, void* stream);
int evc_moments_bound_site_f32(const float* part, int nsplit, int C, int c_begin, int c_count, int n_ranges, int B,
                               unsigned* bound_bits, unsigned* events, unsigned* site_events, int site, void* stream);

/* y = act(x*coef_a[b][c] + coef_s[b][c]) elementwise on NHWC: the stand-alone form of the fused load.  One pass per
 * tensor instead of once per filter tap inside the convolution (SiLU costs MFMA issue slots there; HBM is cheap).
 * `coef_*` rows have stride ld_coef (0 = C) so a slice of a concat's coefficients can be used; `y` rows have stride
 * ld_out (0 = C) so two tensors can be activated side by side into one buffer (materialised concat). */
int evc_affine_act_nhwc_f32(const float* x, float* y, const float* coef_a, const float* coef_s, int act, int B,
                            int HW, int C, int ld_coef, int ld_out, void* stream);

/* SPADE act-norm of the conditioning-by-normalisation variant of the score network (reference
 * models/better/layerspp.py:152-173 MySPADE.forward + :518-549 get_act_norm.forward with norm == 'spade'):
 *   y = act( [ (x*coef_a[b][c] + coef_s[b][c]) * gmap[pixel][c] + bmap[pixel][c] ] * (1 + scale[row[b]][c]) + shift[row[b]][c] )
 * coef_*: parameter-free GroupNorm coefficients (evc_gn_coeffs_f32 mode 0, eps 1e-6); gmap = 1 + gamma(cond) and
 * bmap = beta(cond): NHWC maps with row stride ld_map (they depend on the conditioning frames only); ss_scale / ss_shift:
 * AdaGN table columns with row stride ld_ss, NULL for the final norm (no time embedding); `row` NULL = row 0.  x is
 * contiguous [B*HW][C]; all pointers may be offset to a channel slice of wider buffers (ld_* are the full widths). */
int evc_spade_act_nhwc_f32(const float* x, float* y, const float* coef_a, const float* coef_s, int ld_coef,
                           const float* gmap, const float* bmap, int ld_map, const float* ss_scale,
                           const float* ss_shift, int ld_ss, const int* row, int act, int B, int HW, int C, int ld_out,
                           void* stream);

/* ---- convolution as implicit GEMM on the matrix cores -----------------------------------------
 * Two arithmetics, both fp32 in / fp32 accumulate (see EVC_ARITH_* above); the packing of the weights selects one:
 *   EVC_ARITH_BF16X6 (default of the Python host): conv_split_rr_kernel for 3x3 filters on tiles made of whole image
 *     rows (W divides 128: every 3x3 layer of the score network and of ELIC's 8..128-wide stages), conv_split_kernel
 *     for everything else (1x1, 5x5, odd widths);
 *   EVC_ARITH_F32: conv_igemm_kernel (v_mfma_f32_32x32x2_f32).
 * Stride-1 "same" convolution (odd KH x KW, zero padding) over the virtual concat [src0 | src1] of
 * NHWC tensors.  Replaces nn.Conv2d 3x3 / 1x1 (models/better/layers.py:89-113), NIN
 * (models/better/layers.py:535-544), nn.Linear (time-embedding MLP, Dense_0) and the ELIC conv
 * stacks (Network.py:106-166).
 *   in   = act_in(src * coef_a + coef_s)            (coef may be NULL; zero padding after act)
 *   out  = act_out((conv(in, w) + bias + res) * out_scale)
 * Weights are pre-packed by evc_conv_pack_weights_f32 into [KH*KW][Ci/16][CoPad][16].
 * C0, C1 must be multiples of 16.  `ws` is a workspace of evc_conv_workspace_bytes() bytes
 * (split-K partial sums; may be NULL when that returns 0). */
typedef struct {
    const float* src0; const float* src1; int C0; int C1;
    int ld0; int ld1;      /* row strides (floats) of src0 / src1; 0 = C0 / C1 (dense). Lets a source be a
                              channel slice of a wider NHWC tensor. Must be multiples of 4. */
    const float* coef_a; const float* coef_s; int act_in;
    const float* w_packed; const float* bias; const float* res; int ld_res;
    float out_scale; int act_out;
    float* out; int ld_out;
    int B; int H; int W; int Co; int KH; int KW;
    int splits;            /* 0 = choose automatically */
    float* stats_out;      /* optional: per-channel moments of `out`, fused into the epilogue, in the layout of
                              evc_chan_stats_f32 with nsplit = evc_conv_stats_splits() ([B][nsplit][Co][2] = {sum, sumsq}
                              of each pixel run). Only honoured when that is > 0; else must be NULL. */
    int arith;             /* EVC_ARITH_*: must match the packing of w_packed */
    const unsigned* in_bound;  /* EVC_ARITH_F16X3 only, optional (NULL otherwise): device word holding the bit pattern of a
                              float S such that every element of src0 / src1 satisfies |x| <= sqrt(S) -- written by
                              evc_gn_coeffs_bound_f32 / evc_moments_bound_f32 from the tensors' moments.  The kernel scales
                              the sources by the power of two that brings sqrt(S) into [64, 128) before the fp16 split and
                              the accumulator by its inverse: lets the fp16 arithmetic take inputs that no GroupNorm has
                              normalised (1x1 skip convolutions, NIN output projections). */
    /* Optional FUSED 1x1 OPERAND (x2_w_packed != NULL; only where evc_conv_fused_1x1_supported() says so: EVC_ARITH_F16X3,
     * 3x3 filters on the row-reuse kernel):
     *     out = act_out((conv(act_in(cat[src0,src1]*a+s), w) + conv1x1(cat[x2_src0,x2_src1], x2_w) + bias + res) * out_scale)
     * = a res-block's Conv_1 plus its 1x1 skip convolution Conv_2 on the block input (reference
     * models/better/layerspp.py:603-624: x = Conv_2(x); return (x + h) / sqrt(2)) in ONE launch and one accumulator:
     * x2's K-steps run first, the accumulators are rescaled by the (power-of-two) ratio of the two operands' scales, the
     * 3x3 K loop continues into them.  x2 is a raw tensor of the output's B x H x W (two sources like src, row strides
     * x2_ld*, 0 = C), x2_w_packed its [Co][x2_C0+x2_C1][1][1] weights packed for EVC_ARITH_F16X3, x2_bound its element
     * bound (as in_bound, required).  `bias` must already hold the sum of both convolutions' biases. */
    const float* x2_src0; const float* x2_src1; int x2_C0; int x2_C1; int x2_ld0; int x2_ld1;
    const float* x2_w_packed; const unsigned* x2_bound;
    int invariant;         /* 0 = the default plan.  1 = BATCH-INVARIANT mode (see below): the plan is a function of the layer
                              (H, W, C0 + C1, fused-operand channels, Co, KH, KW, arith, on-load mode) only, B sizes the grid;
                              in_bound / x2_bound then point to B words, one per sample. */
} evc_conv_args;
int evc_conv_co_pad(int Co);
long long evc_conv_packed_floats(int Co, int Ci, int KH, int KW);
/* w: [Co][Ci][KH][KW] (PyTorch Conv2d layout, device) -> packed (device). */
int evc_conv_pack_weights_f32(const float* w, float* packed, int Co, int Ci, int KH, int KW, void* stream);
/* The same for any arithmetic: EVC_ARITH_F32 -> the layout above (4 bytes per element), EVC_ARITH_BF16X6 ->
 * [KH*KW][Ci/16][3 planes][CoPad][16 bf16] (6 bytes per element), EVC_ARITH_F16X3 -> a 256-byte header (inverse
 * accumulator scale, weight scale) + [KH*KW][Ci/16][2 planes][CoPad][16 fp16] (4 bytes per element). */
long long evc_conv_packed_bytes(int Co, int Ci, int KH, int KW, int arith);
int evc_conv_pack_weights(const float* w, void* packed, int Co, int Ci, int KH, int KW, int arith, void* stream);
/* Process-wide tuning switches of the convolution dispatch (A/B measurements, tests of non-default kernels; results are
 * the same up to fp32 summation order): "wide_tiles" (default 1: 256-pixel row tiles on large unsplit grids), "row_reuse"
 * (default 1: the row-reuse kernel for 3x3 filters), "tail_split" (default 1: K-split tail of 1.x / 2.x-round grids), "wide256"
 * (default 1: conv_wide_kernel, the 256 x 192 one-workgroup-per-CU f16x3 kernel, on grids of at least one full round), "wide_mid"
 * (default 1: the same kernel with a uniform K split on grids below one round), "wide_cut" (default 1: on grids of 129..255 such
 * workgroups every tile is cut into a long and a short K piece so that the idle CUs take the short ones).
 * Returns EVC_EINVAL for an unknown name. */
int evc_conv_set_option(const char* name, int value);
/* Name of the kernel template instance evc_conv2d_nhwc_f32 launches for these arguments, as rocprofv3 --kernel-trace --stats
 * prints it (e.g. "conv_wide_kernel<2, 4, false>"): lets a profile be matched to launches without mirroring the dispatch.
 * Returns the string length (truncated to n - 1), or the error code of the launch for arguments it refuses (see
 * evc_conv_plan_query). */
int evc_conv_kernel_name(const evc_conv_args* a, char* buf, int n);
int evc_conv_choose_splits(const evc_conv_args* a);
int evc_conv_fused_1x1_supported(const evc_conv_args* a);   /* 1: these arguments may carry the fused 1x1 operand */
/* The number of pixel runs per image (H*W/64 or H*W/32) for which the fused moments will be written, when they are
 * available for these arguments (H*W % 64 == 0 and either split-K -- the combine kernel writes them -- or only full
 * tiles), else 0: the caller then runs evc_chan_stats_f32 on the output instead. */
int evc_conv_stats_splits(const evc_conv_args* a);
long long evc_conv_workspace_bytes(const evc_conv_args* a);
int evc_conv2d_nhwc_f32(const evc_conv_args* a, float* ws, void* stream);

/* ---- batch-invariant mode --------------------------------------------------------------------
 * Opt-in per call (evc_conv_args::invariant, the *_sample_* / *_invariant_* entry points below; never process-wide: one
 * process may run default and invariant networks side by side).  In this mode the numbers computed for one sample are a
 * function of that sample's inputs and the weights only -- not of B, of the sample's row or of the other rows:
 *   - convolutions: kernel family, tile, split-K count and boundaries and the unequal cut are those of the default plan of the
 *     same layer at B = 9, without the K-split tail and ignoring evc_conv_set_option; tiles that are not whole fractions of a
 *     sample (H*W % tile != 0) always take the per-element epilogue; the fused moments have one producer and one run length
 *     per layer (evc_conv_stats_splits: 0 = run evc_chan_stats_f32, at every B alike);
 *   - element bounds of the fp16 split: one word PER SAMPLE (bound_bits[b], bound_bits[b * n_ranges + z]); a pixel is scaled
 *     from its own sample's word.  conv_split_rr_kernel / conv_wide_kernel keep one scale per tile, so a bounded or fused
 *     operand needs H*W % tile == 0 there (EVC_EUNSUPPORTED otherwise; evc_conv_fused_1x1_supported says 0); the 1x1
 *     kernel scales per pixel row;
 *   - attention: waves per workgroup and key parts from (heads, N, D) only (the default plan at B = 9, always the
 *     with-workspace one), evc_attention_set_option ignored.
 * The bits of this mode are NOT those of the default mode at any particular B.  evc_invariant_plan_revision() is bumped
 * whenever a change alters them (job streams carry it). */
#define EVC_INVARIANT_REF_BATCH 9      /* the batch whose default plan is the invariant plan (convolutions and attention) */
int evc_invariant_plan_revision(void);
/* The whole plan of a convolution, without a launch: the kernel instance (as evc_conv_kernel_name), the pixel x channel
 * tile, the K split (count, K-steps per split, first chunk of the second piece of an unequal 2-way cut or 0), the K-split
 * tail (pixel tiles, ways; 0 / 1 = none), the fused-moment runs per image (evc_conv_stats_splits) and whether a fused 1x1
 * operand is accepted.
 * The launch and every query (this one, evc_conv_kernel_name, evc_conv_choose_splits, evc_conv_workspace_bytes,
 * evc_conv_stats_splits, evc_conv_fused_1x1_supported) read one resolved plan, so no query describes a launch that cannot
 * happen: for arguments evc_conv2d_nhwc_f32 refuses, the first four return the launch's error code and the last two return 0.
 * Those are: GroupNorm coefficients with an on-load activation other than none / SiLU (EVC_EUNSUPPORTED), an unknown
 * activation code (EVC_EINVAL), in_bound off EVC_ARITH_F16X3 (EVC_EINVAL), more than 32 filter taps, a source beyond 4 GiB, a
 * fused 1x1 operand where fused_1x1 is 0, and batch-invariant mode's one-scale-per-tile refusal (all EVC_EUNSUPPORTED). */
typedef struct {
    char kernel[96];
    int tile_m, tile_n, splits, steps_per_split, cut_chunk, tail_tiles, tail_splits, stats_runs, fused_1x1;
} evc_conv_plan;
int evc_conv_plan_query(const evc_conv_args* a, evc_conv_plan* out);
/* evc_gn_coeffs_bound_site_f32 / evc_moments_bound_site_f32 with one bound word per sample: sample b raises
 * bound_bits[b] (gn_coeffs) or bound_bits[b * n_ranges + z] (moments).  site_events may be NULL. */
int evc_gn_coeffs_bound_sample_f32(const float* part0, int nsplit0, int C0, const float* part1, int nsplit1, int C1, int B,
                                   int HW, int groups, float eps, int mode, const float* gamma, const float* beta,
                                   const float* ss, int ss_ld, const int* row, float* coef_a, float* coef_s,
                                   unsigned* bound_bits, unsigned* events, unsigned* site_events, int site, void* stream);
int evc_moments_bound_sample_f32(const float* part, int nsplit, int C, int c_begin, int c_count, int n_ranges, int B,
                                 unsigned* bound_bits, unsigned* events, unsigned* site_events, int site, void* stream);
/* Attention with the batch-invariant plan.  bounds: NULL = the f32-MFMA kernel, else [B][3] words (q, k, v of each sample)
 * = the fp16-split kernel.  ws: evc_attention_invariant_workspace_bytes() bytes (NULL when that is 0). */
long long evc_attention_invariant_workspace_bytes(int B, int heads, int N, int D);
int evc_attention_invariant_f32(const float* q, const float* k, const float* v, int ld_qkv, float* out, int ld_out, int B,
                                int heads, int N, int D, float scale, const unsigned* bounds, float* ws, void* stream);

/* Measurement hook: the same launch with two hipEvent_t handles (either may be NULL) recorded on `stream` immediately before
 * the convolution kernel and immediately after it, i.e. before the split-K combine kernel: the interval is the convolution
 * kernel's own duration, the figure rocprofv3 --kernel-trace reports for it (bench.py's roofline leg). */
int evc_conv2d_nhwc_profiled_f32(const evc_conv_args* a, float* ws, void* stream, void* ev_start, void* ev_conv_end);

/* ---- NIN / linear projection as a plain GEMM (attention blocks) ------------------------------
 * The 1x1 convolutions of an attention block (q | k | v, and the output projection with its residual) as ONE launch with
 * no K split, no workspace and no second kernel: every output element and every moment entry has one writer and a fixed
 * summation order, so the result does not depend on the grid.  EVC_ARITH_F16X3 only, on the SAME packed weights as
 * evc_conv2d_nhwc_f32 takes for the 1x1 filter (header + [Ci/16][2 planes][CoPad][16] fp16), and to the bit the arithmetic
 * of that convolution's unsplit kernel:
 *     out[m][n] = ((sum_k T(x[m][k]) * w[n][k]) + bias[n] + res[m][n]) * out_scale
 *   T(x) = x * coef_a[b][k] + coef_s[b][k]   (coef_a and coef_s set, in_bound NULL: an affine GroupNorm, operand scale 8), or
 *   T(x) = x                                 (coef_* NULL, in_bound set: a raw operand scaled from its element bound word).
 * x, res, out are dense [B*H*W][Ci / Co / Co].  stats_out (optional): moments of `out`, [B][stats_runs][Co][2] in the
 * layout of evc_chan_stats_f32, stats_runs from evc_nin_gemm_plan_query.  Nothing is clamped: a NaN / inf operand element
 * makes its pixel's output row non-finite, the NaN pattern in the bound word makes the whole output NaN.
 * This is a separate operation: evc_conv2d_nhwc_f32 never launches it and the convolution's plan queries do not know it.
 * A caller asks evc_nin_gemm_supported first and keeps the convolution where it says 0; the launch does not fall back. */
typedef struct {
    const float* x; const float* x1;      /* x1: a second source -- not supported, must be NULL */
    int Ci; int Co;
    const float* coef_a; const float* coef_s;
    const unsigned* in_bound;
    const float* w_packed; int arith;     /* EVC_ARITH_*: the packing of w_packed */
    const float* bias; const float* res;
    float out_scale; int act_out;         /* act_out: EVC_ACT_NONE is the only one supported */
    float* out; float* stats_out;
    int B; int H; int W;
    int tile;                             /* 0 = choose (every caller but an A/B measurement); 22 / 21 / 11 force the 128 x 128 /
                                             128 x 64 / 64 x 64 pixel x channel tile (unsupported where it does not divide) */
} evc_nin_args;
/* The launch's plan: kernel instance as rocprofv3 --kernel-trace prints it, pixel x channel tile (a pure function of
 * B*H*W, Ci, Co and H*W), K stages of 64 channels, pixel runs per image of the fused moments. */
typedef struct {
    char kernel[64];
    int tile_m, tile_n, stages, stats_runs;
} evc_nin_plan;
/* 1 when the launch takes these arguments: an F16X3 pack, a single source, Ci % 64 == 0, Co % 64 == 0, H*W a multiple of the
 * shape's pixel tile, one of the two on-load forms, no output activation -- and (tile == 0 only) the grid is not one the
 * convolution serves better: Co % 192 == 0, H*W % 128 == 0 and at least 256 tiles of 128 pixels x 192 channels, which its
 * unsplit kernel fills the chip with (measured: profiles/NOTES.md).  Reads shapes and which pointers are set, never
 * memory; needs no device.  Everything else gets EVC_EUNSUPPORTED from the launch and the plan query (EVC_EINVAL for a
 * NULL x / w_packed / out or a size <= 0). */
int evc_nin_gemm_supported(const evc_nin_args* a);
int evc_nin_gemm_plan_query(const evc_nin_args* a, evc_nin_plan* out);
int evc_nin_gemm_f32(const evc_nin_args* a, void* stream);

/* ---- 3x3 convolution of the 16 x 16 and 8 x 8 levels: K groups inside the workgroup, one launch -----------------
 * The stride-1 zero-padded 3x3 convolution over the virtual concat [src0 | src1] of dense NHWC tensors, for H = W in {8, 16},
 * EVC_ARITH_F16X3, on the SAME packed weights as evc_conv2d_nhwc_f32 takes:
 *     out = ((conv(T(cat[src0, src1]), w)) + bias + res) * out_scale
 *   T(x) = silu(x * coef_a[b][k] + coef_s[b][k])   (coef_a and coef_s set, act_in = EVC_ACT_SILU), or
 *   T(x) = x                                       (coef_* NULL, act_in = EVC_ACT_NONE: an input the FIR pass has activated);
 *   in_bound (optional, either form): the element bound word of the sources, as in evc_conv_args.
 * The K range is divided over G groups of waves INSIDE each workgroup (contiguous ranges of 16-channel chunks, group
 * partial sums added through the LDS in the fixed order ((g0 + g1) + g2) + ...): no split-K slabs, no workspace, no combine
 * launch, no atomics -- every output element and every moment entry has one writer and a fixed summation order.  That order
 * is not the convolution's, so the two agree to fp32 rounding, not to the bit.  stats_out (optional): moments of `out`,
 * [B][stats_runs][Co][2] in the layout of evc_chan_stats_f32, stats_runs (= H*W / 64) from evc_small_conv_plan_query.
 * Nothing is clamped: a NaN / inf operand element makes the outputs of its 3x3 neighbourhood non-finite, the NaN pattern
 * in the bound word the whole output; like the convolution the launch raises no range event itself (evc_gn_coeffs_bound_f32
 * does, from the moments).
 * This is a separate operation: evc_conv2d_nhwc_f32 never launches it and the convolution's plan queries do not know it.
 * A caller asks evc_small_conv_supported first and keeps the convolution where it says 0; the launch does not fall back. */
typedef struct {
    const float* src0; const float* src1; int C0; int C1;      /* dense: row strides C0 / C1; src1 NULL iff C1 == 0 */
    const float* coef_a; const float* coef_s; int act_in;
    const unsigned* in_bound;
    const float* w_packed; int arith;     /* EVC_ARITH_*: the packing of w_packed */
    const float* bias; const float* res;
    float out_scale; int act_out;         /* act_out: EVC_ACT_NONE is the only one supported */
    float* out; float* stats_out;
    int B; int H; int W; int Co; int KH; int KW;
    const float* x2_w_packed;             /* a fused 1x1 operand (evc_conv_args::x2_*): not supported, must be NULL */
    int invariant;                        /* batch-invariant mode: not supported, must be 0 */
    int variant;                          /* 0 = choose (every caller but an A/B measurement); 1 .. 4 force a kernel instance
                                             (1: 64 pixels x 32 channels, G = 8; 2: 64 x 64, G = 4; 3: 128 x 32, G = 4;
                                             4: 128 x 64, G = 2; 1 / 2 need W = 8, 3 / 4 W = 16); + 16: workgroups in plain
                                             channel-tile-major order instead of one channel tile per XCD */
} evc_small_conv_args;
/* The launch's plan: kernel instance as rocprofv3 --kernel-trace prints it, its number (1 .. 4), pixel x channel tile, K
 * groups, 16-channel chunks, chunks of the longest group (= barriers of the K loop), pixel runs per image of the moments. */
typedef struct {
    char kernel[64];
    int variant, tile_m, tile_n, groups, chunks, rounds, stats_runs;
} evc_small_conv_plan;
/* 1 when the launch takes these arguments: an F16X3 pack, 3x3, H = W in {8, 16}, C0 % 16 == 0, C1 % 16 == 0, Co a multiple of
 * the instance's channel tile, one of the two on-load forms, no output activation, no fused 1x1 operand, default mode --
 * and (variant == 0 only) the shape is one the kernel measured faster on than the convolution (profiles/NOTES.md): at 8 x 8 up
 * to 768 input channels at any batch, more where the last round of Co / 32 x B workgroups on 256 CUs is 3/4 full; at 16 x 16 up
 * to 384 input channels where the 128 x 32 tiles (Co / 32 x 2 B of them) fit one round.  A forced variant is never refused for that.
 * Reads shapes and which pointers are set, never memory; needs no device.  Everything else gets EVC_EUNSUPPORTED from the
 * launch and the plan query (EVC_EINVAL for a NULL src0 / w_packed / out, a size <= 0, src1 and C1 that disagree). */
int evc_small_conv_supported(const evc_small_conv_args* a);
int evc_small_conv_plan_query(const evc_small_conv_args* a, evc_small_conv_plan* out);
int evc_small_conv_f32(const evc_small_conv_args* a, void* stream);

/* ---- multi-head spatial self-attention ------------------------------------------------------
 * out[b][n][h*D + d] = sum_m softmax_m(q[b][n][h].k[b][m][h] * scale) * v[b][m][h][d]
 * q, k, v: [B][N][ld_*] token-major with head h at channel offset h*D; D in {32, 64, 128, 192, 256}
 * (256: always the f32 kernel -- the fp16-split kernel keeps Q and O in registers, D/2 + D/2 of them).
 * Replaces the two einsums + softmax of AttnBlockpp.forward (models/better/layerspp.py:241-246). */
int evc_attention_f32(const float* q, const float* k, const float* v, int ld_qkv, float* out, int ld_out, int B,
                      int heads, int N, int D, float scale, void* stream);
/* The same with a workspace of evc_attention_workspace_bytes() bytes (0 = none needed): launches that would leave
 * SIMDs idle split the KEY range over several workgroups (each leaves an unnormalised partial + running max / sum)
 * and a merge kernel applies the exact online-softmax combination.  Results equal evc_attention_f32 up to fp32
 * rounding of the merge.  The workspace also holds the fp16 kernel's K / V tile images (evc_attention_set_option), so it is
 * non-zero whenever N >= 128 and D is one of 32 / 64 / 128 / 192. */
long long evc_attention_workspace_bytes(int B, int heads, int N, int D);
/* A/B switch: "kv_planes" (default 1) -- evc_attention_f16x3_f32 with >= 512 keys converts K / V ONCE per launch into per-tile
 * images of its LDS layout (a pre-pass into the workspace) and stages them by LDS-DMA, instead of converting every 32-key tile
 * again in every query block.  Same numbers either way.  "f16_min_keys" (default 128): fewest keys for which
 * evc_attention_f16x3_f32 runs the fp16-split kernel (below it the f32-MFMA kernel: B = 9, 64 keys, 4 heads of 192: 26 us vs 40 us).
 * "short_seq" (default 1): N <= 256 keys and D <= 192 run the short-sequence kernels -- ONE launch of 4-wave workgroups, one per
 * (sample, head, 32-query block), whose waves cut the reduction over D of K Q^T and deal out the D / 32 tiles of P V; no key
 * parts, no merge launch, the workspace is not used (evc_attention_workspace_bytes is unchanged).  The arithmetic is chosen as
 * before (f32 MFMA, or the fp16 split from "f16_min_keys" keys on).  0: the kernels and plans used above 256 keys.  B = 9, 4 heads
 * of 192, 64 keys: 26 -> 11 us; 3 heads, 256 keys: 29 -> 27 us.  evc_attention_invariant_f32 ignores all three.
 * Returns EVC_EINVAL for an unknown name. */
int evc_attention_set_option(const char* name, int value);
int evc_attention_ws_f32(const float* q, const float* k, const float* v, int ld_qkv, float* out, int ld_out, int B,
                         int heads, int N, int D, float scale, float* ws, void* stream);

/* The same attention on the fp16 matrix cores (EVC_ARITH_F16X3 scheme: operands scaled by powers of two, 2-way fp16
 * split, three v_mfma_f32_32x32x16_f16 per product, fp32 accumulation and fp32 softmax).  `bounds` = three device words
 * holding the bit patterns of floats Sq, Sk, Sv with |q| <= sqrt(Sq), |k| <= sqrt(Sk), |v| <= sqrt(Sv) elementwise
 * (evc_moments_bound_f32 over the q / k / v channel ranges of the projection's moments).  Same workspace as
 * evc_attention_ws_f32 (pass NULL when evc_attention_workspace_bytes() is 0). */
int evc_attention_f16x3_f32(const float* q, const float* k, const float* v, int ld_qkv, float* out, int ld_out, int B,
                            int heads, int N, int D, float scale, const unsigned* bounds, float* ws, void* stream);

/* The whole plan of an attention launch without a launch (no device needed): the kernel template instance as rocprofv3
 * --kernel-trace prints it up to spacing ("attention_kernel<192,4>", "attention_f16_kernel<192,4,pre>",
 * "attention_short_f16_kernel<64>"), waves per workgroup, key parts and 32-key tiles per part, whether
 * attention_kv_planes_kernel writes K / V tile images first (kv_planes), whether attention_merge_kernel follows (merge), whether
 * it is a short-sequence kernel, the kernel's dynamic LDS, the bytes of the key-part buffers at the head of the workspace (= the
 * offset of the K / V tile images) and what evc_attention_workspace_bytes / evc_attention_invariant_workspace_bytes report for
 * the shape.  The launches are made from the same resolved plan, so the answer is what runs.
 *   invariant = 0, with_bounds = 0, have_ws = 0   evc_attention_f32
 *   invariant = 0, with_bounds = 0, have_ws = 1   evc_attention_ws_f32 with a workspace
 *   invariant = 0, with_bounds = 1                evc_attention_f16x3_f32, have_ws: with a workspace or with NULL
 *   invariant = 1                                 evc_attention_invariant_f32, with_bounds: bounds given or NULL
 * Default mode reflects the current evc_attention_set_option values, invariant mode ignores them.  Arguments the launch refuses
 * give the launch's error code: EVC_EUNSUPPORTED for a head width outside the above, EVC_EINVAL for a size <= 0 and for
 * have_ws = 0 where the entry point asks for a workspace (evc_attention_f16x3_f32 / evc_attention_invariant_f32 with
 * workspace bytes > 0). */
typedef struct {
    char kernel[64];
    int waves, kparts, tiles_per_part, kv_planes, merge, short_seq;
    long long lds_bytes, parts_bytes, ws_bytes;
} evc_attention_plan;
int evc_attention_plan_query(int B, int heads, int N, int D, int with_bounds, int have_ws, int invariant,
                             evc_attention_plan* out);

/* ---- frame axis (pseudo-3-D score network, config.model.arch = unetmorepseudo3d) -----------------
 * Video activations are x[b][n][pixel][c]: an NHWC tensor of B*N images, the N frames of a sample adjacent.  A per-frame Conv2d
 * is then evc_conv2d_nhwc_f32 over B*N images; PseudoConv3d's Conv1d over the frames (reference models/better/layers3d.py:274,
 * 294-297) is evc_conv2d_nhwc_f32 with KH = 3 (or 1), KW = 1 over B "images" of N rows x H*W columns; the 3-D GroupNorm's
 * moments are evc_chan_stats_f32's with N times the pixel runs.  The operations below have no 2-D counterpart. */
/* nn.GroupNorm of AttnBlockpp1d on (B*H*W, C, N) (layers3d.py:89-90,107): per pixel, moments over (C / groups channels x N
 * frames), biased variance, then * gamma[c] + beta[c].  y may alias x. */
int evc_frame_group_norm_f32(const float* x, float* y, const float* gamma, const float* beta, int B, int N, int HW, int C,
                             int groups, float eps, void* stream);
/* Attention over the N <= 8 frames of one pixel (AttnBlockpp1d.forward, layers3d.py:112-118): q | k | v are channel ranges
 * [0, C) | [C, 2C) | [2C, 3C) of qkv rows of stride ld_qkv; per (pixel, head) softmax_i(q_t . k_i * scale) applied to v. */
int evc_frame_attention_f32(const float* qkv, int ld_qkv, float* out, int ld_out, int B, int N, int HW, int C, int heads,
                            float scale, void* stream);
/* The 1x1 "converter" convolution over the frame axis (reference models/better/ncsnpp_more.py:213-216,226-228,328-335,
 * 344-351): y[b][m][j] = sum_n w[m][n] * x[b][n][j] + bias[m], j < inner = H*W*C (multiple of 4), N, M <= 8. */
int evc_frame_mix_f32(const float* x, float* y, const float* w, const float* bias, int B, int N, int M, long long inner,
                      void* stream);

/* The temporal taps of nn.Conv3d (config.model.arch = unetmore3d, reference models/better/layers3d.py:225-243) side by side
 * along the channels: y[b][n][pixel][kt*C + c] = x[b][n + kt - 1][pixel][c], zeros beyond a sample's first / last frame,
 * kt = 0, 1, 2.  The 3 x 3 x 3 convolution is then evc_conv2d_nhwc_f32 (KH = KW = 3) over B*N images with 3C input channels
 * and the weight (Co, Ci, kt, kh, kw) read as (Co, kt*Ci + ci, kh, kw).  x must already be activated (zeros stay zeros). */
int evc_frame_taps_f32(const float* x, float* y, int B, int N, int HW, int C, void* stream);

/* ---- sampler steps (elementwise, flat over n floats) ---------------------------------------- */
/* DDPM ancestral step (models/__init__.py:289-330):
 *   x0 = k1*(x - k2*e); clip; x = c1*x0 + c2*x (+ sigma*noise when noise != NULL). */
int evc_ddpm_step_f32(float* x, const float* e, const float* noise, long long n, float k1, float k2, float c1,
                      float c2, float sigma, int clip, void* stream);
/* DDIM step (models/__init__.py:163-166): x = c1*clip(k1*(x - k2*e)) + c2*e. */
int evc_ddim_step_f32(float* x, const float* e, long long n, float k1, float k2, float c1, float c2, int clip,
                      void* stream);
/* y = x + alpha*e  (final denoise call, models/__init__.py:333-335, with alpha = -sqrt(1-a)). */
int evc_axpy_f32(const float* x, const float* e, float* y, long long n, float alpha, void* stream);
/* PNDM transfer (models/pndm.py:19-33): y = clip(x + d*(cx*x - ce*e)). */
int evc_pndm_transfer_f32(const float* x, const float* e, float* y, long long n, float d, float cx, float ce,
                          int clip, void* stream);
/* y = w0*e0 + w1*e1 + w2*e2 + w3*e3 (Runge-Kutta / Adams-Bashforth combination, pndm.py:15,47). */
int evc_lincomb4_f32(const float* e0, const float* e1, const float* e2, const float* e3, float* y, long long n,
                     float w0, float w1, float w2, float w3, void* stream);
/* data_transform / inverse_data_transform (city_sender.py:232-244, function.py:73-82):
 * y = x*mul + add, optionally clamped to [lo, hi]. */
int evc_scale_clamp_f32(const float* x, float* y, long long n, float mul, float add, int clamp, float lo, float hi,
                        void* stream);

/* ---- ELIC helpers ---------------------------------------------------------------------------- */
/* out = a * sigmoid(b) + x (AttentionBlock.forward, ELICUtilis/layers/layers.py:247-252). */
int evc_gate_residual_f32(const float* a, const float* b, const float* x, float* out, long long n, void* stream);
/* GaussianConditional.build_indexes on the checkerboard half of a slice (Network.py:488-496):
 * for the anchor (parity 0) or non-anchor (parity 1) sites of scales [B][H][W][ld] at channel
 * offset c0..c0+C, write idx[b][c][h][w/2] = #table entries logic of compressai build_indexes and the
 * matching means[b][c][h][w/2]. */
int evc_elic_gather_params_f32(const float* ms, int ld, int mean_off, int scale_off, int C, int B, int H, int W,
                               int parity, const float* scale_table, int n_scales, int* idx, float* means,
                               void* stream);
/* y_hat[b][h][w][c0 + c] = symbols[b][c][h][w/2] + means (checkerboard sites of `parity`); other sites
 * untouched (Network.py:498-499, 523-524). */
int evc_elic_scatter_symbols_f32(const int* symbols, const float* means, float* y_hat, int ld, int c0, int C,
                                 int B, int H, int W, int parity, void* stream);
/* Encoder side (Network.py:399, 423 via compressai quantize "symbols"): symbols[b][c][h][w/2] =
 * round_half_even(y[b][h][w][c0 + c] - means[b][c][h][w/2]) at the checkerboard sites of `parity`. */
int evc_elic_quantize_f32(const float* y, int ld, int c0, const float* means, int C, int B, int H, int W,
                          int parity, int* symbols, void* stream);

/* ---- ELIC rate estimation (csrc/rate.hip): TestModel.inference (Network.py:534-640), the rate without an entropy coder --------
 * Both kernels run one workgroup per sample and add -log2(likelihood) over the sample's sites in an order that depends on
 * (C, H, W) only (per-lane strided partial sums in double, wave shuffle tree, fixed pass over the wave totals; a plain store, no
 * atomics): bits[b] is the same pattern whatever else is in the batch.  compressai's bounds are torch.max(x, bound): a NaN in
 * y, a mean, a scale or z gives NaN bits for that sample (and torch's NaN in y_hat / z_hat), +-inf in y - mean the floor value
 * -log2(1e-9); other samples are unaffected.  Caller's stream, no allocation.
 *
 * One (slice, parity) pass of the Gaussian-conditional model.  Replaces evc_elic_gather_params_f32 + evc_elic_quantize_f32 +
 * evc_elic_scatter_symbols_f32 + the host range coder of that pass: GaussianConditional.forward in eval mode (compressai 1.1.5:
 * quantize "dequantize", _likelihood with its fp32 erfc difference, scale bound 0.11 and likelihood bound 1e-9).  At the
 * checkerboard sites of `parity` (same sites as above) of ms [B][H][W][ld] = [.. means at mean_off .. scales at scale_off ..] and
 * y [B][H][W][ld_y] at channels c0 .. c0+C: y_hat[b][h][w][c0 + c] = rint(y - mean) + mean (bit-identical to
 * evc_elic_scatter_symbols_f32 of the coded path; all other elements untouched), bits[b] = sum of -log2 p. */
int evc_elic_rate_pass_f32(const float* ms, int ld, int mean_off, int scale_off, int C, const float* y, int ld_y, int c0,
                           int B, int H, int W, int parity, float* y_hat, double* bits, void* stream);
/* The factorised density of the hyper-latent.  Replaces EntropyBottleneck.compress / decompress on the host (entropy.py
 * EntropyBottleneckCodec + the range coder): EntropyBottleneck.forward in eval mode (compressai 1.1.5, filters (3,3,3,3)).
 * z, z_hat [B][H][W][ld] (C <= ld channels used), medians [C], density [C][58]: per channel softplus(matrix), bias, tanh(factor)
 * of the five layers packed 3+3+3, 3 x (9+3+3), 3+1 (matrices row-major [out][in]; entropy.pack_density).
 * z_hat = rint(z - median) + median, bits[b] = sum of -log2 max(|sigmoid(s*upper) - sigmoid(s*lower)|, 1e-9) with lower / upper =
 * logits_cumulative(z_hat -+ 0.5), s = -sign(lower + upper). */
int evc_bottleneck_rate_f32(const float* z, int ld, int C, int B, int H, int W, const float* medians, const float* density,
                            float* z_hat, double* bits, void* stream);

/* ---- ELIC stride-2 convolutions, polyphase form (csrc/stride2.hip) ----------------------------------------------
 * compressai deconv() = ConvTranspose2d(k 5, stride 2, padding 2, output_padding 1) and conv() = Conv2d(k 5, stride 2,
 * padding 2) (reference Network.py:88-138).  Exactly the same sums as the direct forms, as ONE 3x3 stride-1 convolution
 * (evc_conv2d_nhwc_f32) on the low-resolution side plus a layout pass: 36 MACs per low-resolution pixel and channel pair
 * instead of the 100 of zero-insertion / decimation around a 5x5 "same" convolution.
 *   evc_deconv5x5s2_phase_weights_f32: ConvTranspose2d weight wt [Ci][Co][5][5] -> wp [4*Cp][CiPad][3][3] (phase-major
 *       output channels, zero taps where a phase has two; Cp >= Co, CiPad >= Ci), to be packed by evc_conv_pack_weights.
 *   evc_conv5x5s2_phase_weights_f32: Conv2d weight w [Co][Ci][5][5] -> wq [Co][4*Cq][3][3] over the space-to-depth input.
 *   evc_depth_to_space2_f32 / evc_space_to_depth2_f32: the layout passes (pure permutations, zero padding channels).
 *   evc_deconv5x5s2_f32: x [B][H][W][Ci] -> out [B][2H][2W][Co]; bias4 [4*Cp] = the bias repeated per phase.
 *   evc_conv5x5s2_f32:   x [B][2Ho][2Wo][ld_in] (first Ci channels) -> out [B][Ho][Wo][Co]. */
int evc_deconv5x5s2_phase_weights_f32(const float* wt, float* wp, int Ci, int Co, int Cp, int CiPad, void* stream);
int evc_conv5x5s2_phase_weights_f32(const float* w, float* wq, int Co, int Ci, int Cq, void* stream);
int evc_depth_to_space2_f32(const float* in, int ld_in, int Cp, float* out, int C, int B, int H, int W, void* stream);
int evc_space_to_depth2_f32(const float* in, int ld_in, int C, float* out, int ld_out, int Cq, int B, int H, int W,
                            void* stream);
long long evc_deconv5x5s2_workspace_bytes(int B, int H, int W, int Cp);
int evc_deconv5x5s2_f32(const float* x, const void* w_packed, int arith, const float* bias4, float* out, float* ws, int B,
                        int H, int W, int Ci, int Co, int act_out, void* stream);
long long evc_conv5x5s2_workspace_bytes(int B, int Ho, int Wo, int Ci);
int evc_conv5x5s2_f32(const float* x, int ld_in, const void* w_packed, int arith, const float* bias, float* out, float* ws,
                      int B, int Ho, int Wo, int Ci, int Co, int act_out, void* stream);

/* ---- LPIPS (AlexNet, v0.1): the perceptual distance of the sender's decision rule ------------------------------
 * Replaces lpips.LPIPS(net='alex') as built by city_sender.py:302 and called by decide_5to5_lpips (:376-406); the
 * algorithm is the one vendored in models/networks_basic.py:62-93 (PNetLin.forward, ScalingLayer), models/eval_models.py:35-37
 * (normalize_tensor) and models/pretrained_networks.py:56-94 (AlexNet slices), restated in oracle/lpips.py.  The five convolutions run on evc_conv2d_nhwc_f32; these
 * are the other pieces (csrc/lpips.hip):
 *   evc_im2col_nchw_f32   x (N, C, H, W) NCHW -> out (N, Ho, Wo, ld_out) rows of KH*KW patches in (c, ky, kx) order, the
 *                         columns C*KH*KW .. ld_out-1 zero; optional per-channel (x - shift[c]) / scale[c] (the ScalingLayer)
 *                         applied before the zero padding, as the convolution that follows would see it.  Ho = (H + 2 pad -
 *                         KH) / stride + 1.  Turns the stride-4 11x11 first convolution into a 1x1 convolution.
 *   evc_maxpool3s2_nhwc_f32   MaxPool2d(3, stride 2), no padding, floor: (N, H, W, C) -> (N, (H-3)/2+1, (W-3)/2+1, C), C % 4 == 0.
 *   evc_lpips_layer_f32   one feature tap: dist[n] (+)= mean over pixels of sum_c lin_w[c] * (f0/(|f0|_2 + 1e-10) -
 *                         f1/(|f1|_2 + 1e-10))^2, norms over the channels of a pixel; f0, f1: (N, HW, C) NHWC. */
int evc_im2col_nchw_f32(const float* x, float* out, int N, int C, int H, int W, int KH, int KW, int stride, int pad, int ld_out,
                        const float* shift, const float* scale, void* stream);
int evc_maxpool3s2_nhwc_f32(const float* x, float* out, int N, int H, int W, int C, void* stream);
int evc_lpips_layer_f32(const float* f0, const float* f1, const float* lin_w, float* dist, int N, int HW, int C, int accumulate,
                        void* stream);

/* ---- LPIPS, the whole family: VGG16 and SqueezeNet 1.1 backbones, spatial maps (csrc/lpips.hip) ----
 * The reference vendors all three networks (models/networks_basic.py:25-88 PNetLin with pnet_type vgg / alex / squeeze,
 * models/pretrained_networks.py:5-134 the slices, weights/v0.1/{alex,vgg,squeeze}.pth the trained linear layers) and its
 * benchmark metric is the spatial form (fvd_utils/calculate_lpips.py:9-58: lpips.LPIPS(net=..., spatial=True) on frames in
 * [-1, 1], .mean() of the map).  The convolutions run on evc_conv2d_nhwc_f32 and evc_im2col_nchw_f32; these are the rest:
 *   evc_maxpool2d_nhwc_f32   MaxPool2d(k, stride) without padding, k in {2, 3}: (2, 2) floor of torchvision vgg16.features
 *                         4/9/16/23 and (3, 2, ceil_mode=True) of squeezenet1_1.features 2/5/8 (pretrained_networks.py:5-53,96-134).
 *                         (N, H, W, C) -> (N, Ho, Wo, C) with torch's output size: floor or ceil of (H - k) / stride, + 1, and
 *                         in ceil mode one less when the last window would start beyond the input.  Window elements beyond
 *                         the input are skipped; a NaN is kept as torch keeps it.  C % 4 == 0 (16-byte accesses); H, W >= k, or in ceil mode >= k - stride + 1.
 *   evc_lpips_map_f32     map[n][p] = sum_c lin_w[c] * (f0/(|f0|_2 + 1e-10) - f1/(|f1|_2 + 1e-10))^2 for every pixel p of every
 *                         pair n (networks_basic.py:68-70 + NetLinLayer :100-107, eval_models.py:35-37); f0, f1: (N, HW, C)
 *                         NHWC, 16-byte aligned like lin_w, C a multiple of 64 from 64 to 512.  The grid runs over all N * HW
 *                         pixels, 16 lanes per pixel; each element is read once.  A NaN / inf channel makes its pixel NaN.
 *   evc_lpips_map_mean_f32   dist[n] (+)= mean_p map[n][p] (spatial_average, networks_basic.py:15-16); the summation order
 *                         depends on HW only.
 *   evc_lpips_upsample_add_f32   out[n] (+)= bilinear(map[n] (h, w) -> (H, W)), align_corners = False, torch's float32 formula:
 *                         scale = h / H, source index max((dst + 0.5) * scale - 0.5, 0), upper neighbour clamped to h - 1.
 *                         lpips 0.1.4 (requirements.txt:66) up-samples with nn.Upsample(size=(H, W)); the vendored
 *                         networks_basic.py:18-22 passes scale_factor = H / h instead, which is the same map wherever that
 *                         form gives an (H, W) output at all, up to the rounding of 1 / (H / h) against h / H.  NaN and inf
 *                         propagate as in torch (a zero weight times inf is NaN).
 * accumulate: 0 stores, 1 adds to what dist / out hold.  EVC_EINVAL before any launch for a null pointer, a size <= 0, a
 * channel count or k outside the above. */
int evc_maxpool2d_nhwc_f32(const float* x, float* out, int N, int H, int W, int C, int k, int stride, int ceil_mode, void* stream);
int evc_lpips_map_f32(const float* f0, const float* f1, const float* lin_w, float* map, int N, int HW, int C, void* stream);
int evc_lpips_map_mean_f32(const float* map, float* dist, int N, int HW, int accumulate, void* stream);
int evc_lpips_upsample_add_f32(const float* map, float* out, int N, int h, int w, int H, int W, int accumulate, void* stream);

/* ---- I3D (InceptionI3d(400), the feature network of the Frechet video distance) ----------------------------------
 * Replaces the detector of calculate_fvd (city_sender.py:264-279, called per job at :575-589): preprocess_single
 * (models/fvd/fvd.py: bilinear resize, align_corners=False, of the shorter side to R = 224, the other side ceil-ed, centre
 * crop R x R, (x - 0.5) * 2) and InceptionI3d.forward (models/fvd/pytorch_i3d.py:316-327) with TensorFlow-"same" zero padding
 * everywhere (compute_pad, :9-34 and :71-99: pad = max(k - s, 0) when s divides the size, else max(k - size % s, 0); the
 * front gets pad / 2, the back the rest).  Activations are NTHWC: B*T images of H x W x C.  The 1x1x1 units and the 3x3x3
 * units (after evc_frame_taps_f32) run on evc_conv2d_nhwc_f32 with BatchNorm folded into weight and bias; these are the other
 * pieces (csrc/i3d.hip):
 *   evc_i3d_stem_im2col_f32   clips x (B, T, C, H, W) in [0, 1] -> out (nf, Ho, Wo, ld_out): the rows of output frames
 *                         f_begin .. f_begin + nf - 1 (flattened f = b*To + t) of the KT x KH x KW stride-(ST, SH, SW) first
 *                         convolution (Conv3d_1a_7x7, pytorch_i3d.py:209-211) over the preprocessed clip, in (c, kt, ky, kx)
 *                         order, columns C*KT*KH*KW .. ld_out-1 zero.  The resize to Hr x Wr, the crop at ((Hr - R) / 2,
 *                         (Wr - R) / 2), the scaling and the same padding of the R x R crop are applied while sampling; the
 *                         resized video is never written.  To = ceil(T / ST), Ho = ceil(R / SH), Wo = ceil(R / SW); the
 *                         caller's `out` holds nf * Ho * Wo * ld_out floats (that is the workspace bound: chunk nf to fit it).
 *                         The convolution is then a 1x1 one over ld_out channels.
 *   evc_maxpool3d_same_nthwc_f32   MaxPool3dSamePadding (pytorch_i3d.py:7-34): window KT x KH x KW, strides ST, SH, SW,
 *                         zero padding (the padding takes part in the max) -> (B, ceil(T/ST), ceil(H/SH), ceil(W/SW), C),
 *                         C % 4 == 0.  Exactly F.max_pool3d(F.pad(x, same)).
 *   evc_i3d_head_f32      the logits of pytorch_i3d.py:322-327: AvgPool3d((KT, H, W), stride 1) over x (B, T, H*W, C) -- the
 *                         window covers the whole H x W frame -- the 1x1x1 logits unit (w: (Co, C) row-major, bias: (Co,) or
 *                         NULL) and the mean over the T - KT + 1 windows, as one linear map: frame t is weighted by the number
 *                         of windows holding it over KT * HW * (T - KT + 1).  out: (B, Co).  C <= 2048, T >= KT. */
int evc_i3d_stem_im2col_f32(const float* x, float* out, int B, int T, int C, int H, int W, int Hr, int Wr, int R, int KT, int KH,
                            int KW, int ST, int SH, int SW, int f_begin, int nf, int ld_out, void* stream);
int evc_maxpool3d_same_nthwc_f32(const float* x, float* out, int B, int T, int H, int W, int C, int KT, int KH, int KW, int ST,
                                 int SH, int SW, void* stream);
int evc_i3d_head_f32(const float* x, const float* w, const float* bias, float* out, int B, int T, int HW, int C, int Co, int KT,
                     void* stream);

/* ---- GDN (not on the decode path: g_s / g_a contain none) ---------------------------------
 * y = x * rsqrt(beta + gamma . x^2) (inverse: * sqrt) -- GDN.forward, ELICUtilis/layers/gdn.py:62-77; simplified != 0:
 * y = x / (beta + gamma . |x|) -- GDN1.forward, :95-106.  x, out: NHWC with C % 16 == 0; gamma_packed = the
 * re-parametrised (C, C) gamma packed as a 1x1 convolution weight by evc_conv_pack_weights (EVC_ARITH_F32 or _BF16X6);
 * beta: the re-parametrised (C,) vector; ws: evc_gdn_workspace_bytes() bytes. */
long long evc_gdn_workspace_bytes(int B, int H, int W, int C);
int evc_gdn_f32(const float* x, const void* gamma_packed, int arith, const float* beta, float* out, float* ws, int B,
                int H, int W, int C, int inverse, int simplified, void* stream);

/* ---- Noise specification N1: the replayable noise of the job streams (csrc/noise.hip) -------
 * One launch fills the noise of one sampler step for a batch; every sample draws from its own counter-based stream, so its
 * numbers depend on its key only, not on its row in the batch or on B.  out: [B][n] fp32, n % 4 == 0 (the sample's element
 * count, 15*H*W for a chunk); keys: device array [B][2] = (stream id, start frame).  Philox4x32-10 with key = (seed low 32
 * bits, seed high 32 bits) and counter = (j, step, start frame, stream id), j = index of the 4-element block inside the
 * sample; step 0 is x_T, step i + 1 the noise of sampler step i.  The block's words w0..w3 give elements 4j .. 4j+3:
 * u = ((w >> 9) + 0.5) * 2^-23, r = sqrt(-2 ln u(w0)), theta = 2 pi u(w1) -> r cos theta, r sin theta; the same from
 * (w2, w3).  raw != 0 writes the four words bit-cast instead of the normals. */
int evc_noise_normal_f32(float* out, const unsigned* keys, int B, long long n, unsigned long long seed, unsigned step,
                         int raw, void* stream);

/* ---- YUV 4:2:0 <-> RGB: the video file boundary (csrc/yuv.hip) ------------------------------
 * The conventions of the reference's codec benchmark: 8-bit (or 10-bit, little-endian 16-bit samples) planar 4:2:0, full-range
 * BT.709, chroma sited at the centre of its 2x2 luma block.  Both calls describe the samples as ONE device byte buffer of
 * `bytes` bytes: frame n starts at byte first + n * frame_stride, its Y / U / V planes at off_y / off_u / off_v from there
 * (Y: H x W samples, U and V: H/2 x W/2, rows contiguous), so an uploaded piece of a raw .yuv file or of a Y4M file (a
 * "FRAME\n" marker before every frame) is converted where it lies.  No alignment is asked of the offsets.  N <= 65535 frames
 * per launch, H and W even and >= 2, bits 8 or 10, every plane inside the buffer: anything else returns EVC_EINVAL before a launch.
 *   evc_yuv420_to_rgb   ycbcr2rgb(yuv_420_to_444(frame, mode).true_divide(max_val)), benchmark/fvd_utils/bench_uvg.py:479 with
 *                       yuv_420_to_444 (:345-382; benchmark/transform.py:110-147) and ycbcr2rgb (:384-402; transform.py:47-65):
 *                       the raw chroma samples are up-sampled x2 as torch's F.interpolate does (EVC_YUV_NEAREST, _BILINEAR,
 *                       _BICUBIC; align_corners=False, border indices clamped, bicubic A = -0.75), all three planes divided by
 *                       maxv = 2^bits - 1, then r = y + (2 - 2 Kr)(cr - 0.5), b = y + (2 - 2 Kb)(cb - 0.5), g = (y - Kr r - Kb b) /
 *                       Kg with K = 0.2126 / 0.7152 / 0.0722.  out: (N, 3, H, W) NCHW; out_u8 == 0: float32, unclamped (what
 *                       the reference feeds LPIPS and FVD); out_u8 != 0: uint8 = rint(clamp(rgb * 255, 0, 255)), round half to
 *                       even (bench_uvg.py:487; the --data_npy convention).
 *   evc_rgb_to_yuv420   rgb (N, 3, H, W) float32 in [0, 1] -> samples: rgb2ycbcr (transform.py:26-44), chroma = the 2x2 average
 *                       (yuv_444_to_420, :78-107, avg_pool), sample = rint(clamp(v * maxv, 0, maxv)), round half to even.  A
 *                       pixel with a NaN or an infinity writes 0 to its luma sample and to the chroma samples of its 2x2 block
 *                       and ORs EVC_RANGE_NONFINITE into *events (a device word, never NULL); nothing else is saturated
 *                       beyond the clamp. */
#define EVC_YUV_NEAREST 0
#define EVC_YUV_BILINEAR 1
#define EVC_YUV_BICUBIC 2
int evc_yuv420_to_rgb(const unsigned char* src, long long src_bytes, long long first, long long frame_stride, long long off_y,
                      long long off_u, long long off_v, int N, int H, int W, int bits, int mode, void* out, int out_u8,
                      void* stream);
int evc_rgb_to_yuv420(const float* rgb, unsigned char* dst, long long dst_bytes, long long first, long long frame_stride,
                      long long off_y, long long off_u, long long off_v, int N, int H, int W, int bits, unsigned* events,
                      void* stream);

/* ---- Pillow's 8-bit resize: fitting a source frame to the model (csrc/resample.hip) ----------
 * PIL.Image.resize on 8 bits per channel is two integer passes, horizontal then vertical, each rounded to uint8; these are
 * the passes.  src: `planes` planes of `rows` x `cols` uint8, plane p at src + p * plane_stride, its row r at + r * row_stride
 * (bytes; row_stride >= cols, no alignment asked), so a crop of a larger image is a pointer offset plus the image's strides.
 * bounds: n_out x 2 ints (xmin, n), coeffs: n_out x ksize ints, both ON THE DEVICE and the caller's (lib.resample_tables): output
 * index i along the filtered axis is clamp((2^21 + sum_{x < n} src[xmin + x] * coeffs[i][x]) >> 22, 0, 255), int32 throughout,
 * arithmetic shift.  The caller guarantees 0 <= xmin, n <= ksize, xmin + n <= the axis' length and that the sum fits int32 (a
 * window is held inside the axis whatever the table says; no byte outside the planes is read).  dst is packed.  Neither call
 * allocates; a bad shape (a null pointer, a size <= 0 or above 2^24, row_stride < cols, overlapping planes) returns
 * EVC_EINVAL (negative) before any launch.  No floats, no atomics: an output byte depends on its own row (column) and the
 * tables only, not on the other planes of the launch.
 *   evc_resample_h_u8   along the contiguous axis: dst (planes, rows, n_out)
 *   evc_resample_v_u8   along the row axis:        dst (planes, n_out, cols) */
int evc_resample_h_u8(const unsigned char* src, int planes, int rows, int cols, long long plane_stride, long long row_stride,
                      const int* bounds, const int* coeffs, int ksize, int n_out, unsigned char* dst, void* stream);
int evc_resample_v_u8(const unsigned char* src, int planes, int rows, int cols, long long plane_stride, long long row_stride,
                      const int* bounds, const int* coeffs, int ksize, int n_out, unsigned char* dst, void* stream);

/* ---- Whole frames: overlapping tiles of the model's size, cut and blended (csrc/tile.hip) ------
 * A frame larger than the model is coded as ny x nx overlapping S x S tiles, tile t = ty * nx + tx at rows oy[ty] .. oy[ty] + S - 1
 * and columns ox[tx] .. ox[tx] + S - 1 (video_io.tile_grid computes the origins; the reference has no counterpart).  The origins
 * are passed twice: oy_host / ox_host (ny / nx ints in host memory) are what is checked, oy / ox are the same values ON THE
 * DEVICE and the caller's, what the kernels read -- held inside [0, max(L - S, 0)] whatever they say, so no byte outside the
 * buffers is read.  Neither call allocates; EVC_EINVAL before any launch for a null pointer, a size (N, H, W, S, ny, nx) <= 0
 * or above 2^24, an origin outside [0, max(L - S, 0)] or origins that are not strictly increasing (so an axis with L <= S has
 * one tile, at 0).
 *   evc_tile_grid_check   the checks alone, for a caller that sizes buffers by them.  cover != 0 adds what the blend asks.
 *   evc_tile_gather_u8    src (N, 3, H, W) uint8 -> dst (ny * nx, N, 3, S, S) uint8, packed:
 *                         dst[t][n][c][y][x] = src[n][c][min(oy[ty] + y, H - 1)][min(ox[tx] + x, W - 1)] -- a copy; the samples
 *                         past the end of an axis shorter than S repeat its last one.  16-byte accesses where S % 16 == 0 and
 *                         the source address allows, bounds-checked bytes elsewhere.
 *   evc_tile_blend_f32    tiles (ny * nx, N, 3, S, S) fp32 -> out (N, 3, H, W) fp32.  With the integer tent t(i) = min(i + 1,
 *                         S - i), an output pixel (y, x) visits the tiles that cover it in ascending t, at local (ly, lx) = (y -
 *                         oy[ty], x - ox[tx]): acc = acc + float(t(ly) * t(lx)) * v in fp32 (product rounded, then the sum; no
 *                         contraction), den = the integer sum of the weights, out = acc / float(den), IEEE division.  Also
 *                         EVC_EINVAL unless every pixel is covered: first origin 0, last max(L - S, 0), steps of at most S.
 *                         The padding samples of an axis shorter than S are never read.  Nothing is clamped: a NaN / inf in a
 *                         tile reaches exactly the pixels that tile covers.  No atomics; one thread owns 4 adjacent pixels (one
 *                         16-byte store, W % 4 == 0) or one: a frame's bits depend on its own tiles and the grid only, not on
 *                         N, its place in the batch or the other frames.  Tiles (T, N, C, S, S) with C % 3 == 0 are, bit for
 *                         bit, the (T, N * C / 3, 3, S, S) this entry takes: planes are blended one by one.
 *   evc_tile_gather_f32   the gather for fp32 planes of any channel count C (1 .. 2^24): src (N, C, H, W) -> dst (ny * nx, N, C,
 *                         S, S), packed, by the same formula -- a copy of 32-bit words: NaN / inf pass through with their bits,
 *                         nothing is clamped.  One kernel for every shape: a thread owns 4 consecutive destination floats and
 *                         moves them as one 16-byte load and store where they lie in one tile row, their source columns lie
 *                         inside the row and both addresses are 16-byte aligned; elsewhere (odd W, origins or S that are no
 *                         multiples of 4, edge replication) float by float under the clamp.  No atomics; a sample's tiles do
 *                         not depend on N.  (Joint generation, DESIGN.md section 8c: tiled.py gathers the noisy state and the
 *                         conditioning frames of a canvas with it.) */
int evc_tile_grid_check(int N, int H, int W, int S, int ny, int nx, const int* oy_host, const int* ox_host, int cover);
int evc_tile_gather_u8(const unsigned char* src, int N, int H, int W, int S, int ny, int nx, const int* oy_host,
                       const int* ox_host, const int* oy, const int* ox, unsigned char* dst, void* stream);
int evc_tile_blend_f32(const float* tiles, int N, int H, int W, int S, int ny, int nx, const int* oy_host, const int* ox_host,
                       const int* oy, const int* ox, float* out, void* stream);
int evc_tile_gather_f32(const float* src, int N, int C, int H, int W, int S, int ny, int nx, const int* oy_host,
                        const int* ox_host, const int* oy, const int* ox, float* dst, void* stream);

/* ---- SSIM: the structural similarity of the reference's metric helpers (csrc/ssim.hip) ------
 * ssim() of fvd_utils/calculate_ssim.py:6-23 for N pairs of planes.  a, b: N contiguous planes of H x W fp32 each, values
 * in [0, 1]; taps11: the 11 window taps in float64 ON THE DEVICE (the host computes cv2.getGaussianKernel(11, 1.5)); c1, c2:
 * the stabilisers (0.01^2, 0.03^2 in the reference); out[N]: the mean of each plane's SSIM map over the valid region
 * (H - 10) x (W - 10).  The inputs are widened to double and everything after that is double: the separable filter (11 taps
 * along a row, then 11 along a column) of x1, x2, x1^2, x2^2, x1 x2, the map ((2 mu1 mu2 + c1)(2 s12 + c2)) / ((mu1^2 + mu2^2
 * + c1)(s1 + s2 + c2)) with s = E[.] - mu mu, evaluated operation by operation, and its sum.  The filtered maps stay on
 * the chip; per-tile sums go to ws (evc_ssim_workspace_bytes(N, H, W) bytes, 8-byte aligned) and are added per plane in a
 * fixed order by a second launch: a plane's value depends on its own samples and (H, W) only, bit for bit -- not on N, on
 * its place in the batch or on the other planes.  Nothing is clamped or dropped: a NaN or an infinity in a plane makes that
 * plane's value NaN and touches no other plane.  EVC_EINVAL for H < 11, W < 11, N < 0 or (N > 0) a NULL pointer; N == 0
 * launches nothing and returns EVC_OK.  N * H * W may exceed 2^31. */
long long evc_ssim_workspace_bytes(int N, int H, int W);
int evc_ssim_planes_f32(const float* a, const float* b, int N, int H, int W, const double* taps11, double c1, double c2,
                        double* out, void* ws, void* stream);

/* ---- MS-SSIM: the levels of pytorch_msssim.ms_ssim (csrc/msssim.hip) -----------------------
 * For N pairs of planes (a, b: N contiguous planes of H x W fp32 each, values in [0, 1]) and `levels` pyramid levels,
 * out[N][levels][2]: per level the mean of the SSIM map and the mean of its contrast-structure factor,
 *     cs = (2 s12 + c2) / (s1 + s2 + c2),   ssim = ((2 mu1 mu2 + c1) / (mu1^2 + mu2^2 + c1)) * cs,   s = E[.] - mu mu,
 * over the valid region (H_l - 10) x (W_l - 10) of the 11-tap window taps11 (float64 ON THE DEVICE), evaluated operation by
 * operation in double as evc_ssim_planes_f32 does.  Level l + 1 of both planes is avg_pool2d(kernel 2, stride 2, padding =
 * (H_l % 2, W_l % 2), count_include_pad) of level l: H_{l+1} = (H_l + 1) / 2, an odd axis gets one zero row / column in front
 * and only in front, the divisor is always 4; in double, 0.25 * ((x00 + x01) + (x10 + x11)), kept in float64.  The host
 * raises the numbers to the weights (msssim.py); nothing here is clamped.
 * ws: evc_msssim_workspace_bytes(N, H, W, levels) bytes, 8-byte aligned,
 *     = 8 * N * (2 * sum_{l = 1 .. levels-1} H_l W_l  +  2 * sum_{l = 0 .. levels-1} ceil((H_l - 10) / 16) * ceil((W_l - 10) / 16)):
 * the two float64 pyramids of levels >= 1, then two sums per 16x16 map tile.  levels - 1 pool launches, one tile launch for
 * level 0 (fp32 in) and one for every level above (float64 in), one finishing launch that adds a level's tile sums in an order
 * fixed by (H, W, level) -- seven launches for five levels, whatever N is: no
 * atomics, and a plane's 2 * levels numbers depend on its own samples and (H, W, levels) only, bit for bit -- not on N, on its
 * place in the batch or on the other planes.  A NaN or an infinity makes every level that sees it NaN and touches no other
 * plane.  EVC_EINVAL before any launch for N < 0, levels outside 1 .. 8, min(H, W) <= 10 * 2^(levels-1) (nothing is padded) or
 * (N > 0) a NULL pointer; N == 0 launches nothing and returns EVC_OK.  N * H * W may exceed 2^31. */
long long evc_msssim_workspace_bytes(int N, int H, int W, int levels);
int evc_msssim_levels_f32(const float* a, const float* b, int N, int H, int W, int levels, const double* taps11, double c1,
                          double c2, double* out, void* ws, void* stream);

/* ---- Per-frame squared error: the sum under the sender's PSNR rule (csrc/metric.hip) ---------
 * a, b: n contiguous rows (frames) of `elems` fp32 each; out[i] = sum over frame i of ((double)a - (double)b)^2, i.e.
 * elems times the float64 mse of cal_psnr.  One workgroup per frame; the elements are cut into chunks of four by their
 * index in the frame, thread t of 1024 takes chunks t, t + 1024, ... with one partial per position in the chunk, the
 * partials are added in a fixed order (per thread, wave shuffle tree, the 16 wave totals in turn) and stored plainly: no
 * atomics and no workspace.  The order depends on elems only, so out[i] is the same bit pattern whatever n is, whichever
 * row the frame is and wherever the row starts; any elems >= 1 is taken, a chunk is fetched with one 16-byte load where its
 * address allows and with 4-byte loads elsewhere (rows of odd elems, unaligned bases).  The sum differs from the exact one
 * by at most (elems + 1) * 2^-53 relative.  Nothing is clamped or dropped: a NaN or inf - inf in a frame makes that frame's
 * sum NaN, inf against a finite value makes it inf, other frames are unaffected.  Caller's stream, no allocation;
 * EVC_EINVAL before the launch for a null pointer, n <= 0 or elems <= 0.  n * elems may exceed 2^31. */
int evc_frame_sqerr_f64(const float* a, const float* b, int n, long long elems, double* out, void* stream);

/* ---- FID and precision / recall: the Inception-v3 feature network (csrc/inception.hip) ------
 * The reference's evaluation/ package: pytorch-fid's InceptionV3 (inception.py:84-163 the four blocks, :184-328 the patched
 * Inception blocks), the features of fid_PR.py:110-167 and the k-NN precision / recall of pr.py.  Activations are NHWC, the
 * convolutions (BatchNorm folded, ReLU in the epilogue) run on evc_conv2d_nhwc_f32; these are the other pieces.  None of them
 * allocates; every one returns EVC_EINVAL before any launch for a null pointer, a size <= 0 or a channel count it does not take.
 *   evc_inception_stem_im2col_f32   images x (N, 3, H, W) NCHW in [0, 1] -> out (nf, 149, 149, ld_out): the patch rows of
 *                         Conv2d_1a_3x3 (3x3, stride 2, no padding) for the images f_begin .. f_begin + nf - 1, in (c, ky, kx)
 *                         order, columns 27 .. ld_out-1 zero (ld_out >= 27, a multiple of 4).  The patches are taken over
 *                         2 * F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False) - 1 (inception.py:146-153),
 *                         sampled while gathering: the source position of output index dst is the rational ((2 dst + 1) in -
 *                         299) / 598, clamped at 0, the upper neighbour clamped to in - 1, evaluated in integers, so both
 *                         weights of an axis are correctly rounded fp32 values for any in (up-scaling, in = 299, down-scaling
 *                         without antialiasing).  2x - 1 is applied to the four source pixels, then the two horizontal and
 *                         the vertical interpolation: at most seven roundings per value, and in = 299 gives 2x - 1 itself.
 *                         NaN / inf propagate as in torch (a zero weight times inf is NaN).
 *   evc_im2col_nhwc_f32   x (N, H, W, C) -> out (N, Ho, Wo, ld_out): patch rows in (ky, kx, c) order of a KH x KW window with
 *                         strides (SH, SW) and zero padding (PH, PW), Ho = (H + 2 PH - KH) / SH + 1; columns KH*KW*C ..
 *                         ld_out-1 zero.  C % 4 == 0, ld_out % 4 == 0 (16-byte copies: bit exact).  Serves the stride-2 and
 *                         the unpadded 3x3 convolutions of the network (inception.py:86-98, Mixed_6a, Mixed_7a) and any
 *                         filter shape evc_conv_plan_query refuses: the convolution is then 1x1 over ld_out channels with
 *                         weights permuted to (ky, kx, c).
 *   evc_pool3x3s1p1_nhwc_f32   (N, H, W, C) -> the same shape, window 3x3, stride 1, padding 1, C % 4 == 0.  EVC_POOL_AVG:
 *                         F.avg_pool2d(count_include_pad=False) of FIDInceptionA / C / E_1 (inception.py:228, 256, 289): the
 *                         in-image elements added in row-major order in fp32, divided by their count.  EVC_POOL_MAX:
 *                         F.max_pool2d(x, 3, 1, 1) of FIDInceptionE_2 (:324): the padding does not take part, a NaN is kept.
 *   evc_spatial_mean_nhwc_f32   x (N, HW, C) -> out (N, C): AdaptiveAvgPool2d((1, 1)) (inception.py:122, fid_PR.py:159-160);
 *                         C % 4 == 0, N <= 65535.  The order of the additions depends on HW only.
 *   evc_knn_radius_f32    radius2[i] = the (k + 1)-th smallest squared distance from row i of x (n, d) to the rows of x, row i
 *                         included: kthvalue(k + 1) of the self-distance matrix (pr.py:45-46), squared.  1 <= k <= 8, n > k,
 *                         d % 4 == 0.
 *   evc_manifold_hits_f32   flags[i] = 1 when some row j of x (n, d) has squared distance to row i of y (m, d) at most
 *                         radius2[j], else 0 (pr.py:47-52: (dist <= NNk).any(dim=1)).  d % 4 == 0.
 * Both set kernels add the squares of the exact differences (double)a - (double)b in fp64 in an order that depends on d only,
 * compare squared values (no sqrt enters a decision) and write no n x m matrix. */
#define EVC_POOL_AVG 0
#define EVC_POOL_MAX 1
int evc_inception_stem_im2col_f32(const float* x, float* out, int N, int C, int H, int W, int f_begin, int nf, int ld_out,
                                  void* stream);
int evc_im2col_nhwc_f32(const float* x, float* out, int N, int H, int W, int C, int KH, int KW, int SH, int SW, int PH, int PW,
                        int ld_out, void* stream);
int evc_pool3x3s1p1_nhwc_f32(const float* x, float* out, int N, int H, int W, int C, int mode, void* stream);
int evc_spatial_mean_nhwc_f32(const float* x, float* out, int N, int HW, int C, void* stream);
int evc_knn_radius_f32(const float* x, double* radius2, int n, int d, int k, void* stream);
int evc_manifold_hits_f32(const float* y, const float* x, const double* radius2, int* flags, int m, int n, int d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVC_HIP_H */
