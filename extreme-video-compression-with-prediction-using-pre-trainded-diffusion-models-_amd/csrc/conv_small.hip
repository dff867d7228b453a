// conv_small.hip -- the 3x3 convolutions of the 16 x 16 and 8 x 8 levels in ONE launch: K groups inside the workgroup.
//
//   out[m][n] = ((sum_{tap, k} T(src[m + tap][k]) * w[n][k][tap]) + bias[n] + res[m][n]) * out_scale      M = B*H*W, H = W in {8, 16}
//
// Same operand arithmetic as the f16x3 convolution kernels of conv_igemm.hip (transform, power-of-two scale, split2_f16, the
// three cross products of Split<2> per 16-channel K-step into one fp32 accumulator, epilogue in conv_epilogue_full's order),
// on the SAME packed weights.  What differs is the schedule.  At M = 576 .. 2304 pixels these layers need K parallelism to
// fill the chip; the convolution gets it from blockIdx.z splits -- one fp32 slab per split, a combine launch, and workgroups
// whose 17 .. 36 K-steps barely outlive their prologue, with a DMA wait and a barrier on every step.  Here:
//   * a workgroup owns a tile of BM pixels (whole rows of ONE image: the 8 x 8 image, or 8 rows of the 16 x 16 one) x BN
//     channels, and its waves are G K-GROUPS x (WM x WN waves that tile the block, 64 pixels x 32 channels each).  Group g
//     takes the contiguous range [g * ceil(n / G), ...) of the n 16-channel chunks; a chunk is nine K-steps (the taps);
//   * each group stages its chunk's image -- the tile's rows plus a halo row above and below, a zero pixel left and right --
//     ONCE, transformed and split, into its own double-buffered LDS image [buffer][plane][channel half][pixel][16 B] (the
//     layout of conv_wide_kernel: conflict-free fragment reads under any tap shift), and all nine taps read it: one barrier
//     per chunk, 54 MFMAs per wave between barriers.  The next chunk's loads are issued at the top of a chunk and written to
//     the idle buffer in its middle;
//   * a lane's weight fragment is 16 contiguous bytes of the pack, read straight from L2 into registers two K-steps ahead
//     (three register sets; a whole chunk ahead in nine sets measured no faster); the weights never touch the LDS;
//   * when the ranges end, groups 1 .. G-1 pass their accumulators through the LDS and group 0 adds them in the fixed order
//     ((g0 + g1) + g2) + ... -- no atomics, no workspace, no second launch -- then runs the epilogue: scale, bias, residual,
//     out_scale, moments with one writer per (64-pixel run, channel);
//   * a group with fewer chunks than rounds (or none) idles through the remaining barriers and contributes its zeros;
//   * workgroup order: tiles are listed channel-tile-major and XCD x (workgroups go round-robin over the 8 XCDs) takes the
//     x-th eighth of the list, so the re-reads of a weight column by its pixel tiles are served by one XCD's L2.
// This is a separate operation: evc_conv2d_nhwc_f32 and its planner do not know it, and there is no fallback inside.
//
// Replaces nn.Conv2d 3x3 (reference models/better/layers.py:89-113) inside ResnetBlockBigGANppGN (layerspp.py:595-624) at
// the two coarsest levels in default mode.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/evc_hip.h"
#include "split_mfma.h"

namespace {

struct SmallK {
    const float* src0; const float* src1; int C0, C1;
    const float* coef_a; const float* coef_s; const unsigned* in_bound;
    const char* w;            // planes of the pack (behind the header): [tap][chunk][plane][CoPad][16 fp16]
    const float* w_hdr;       // [0] = 1 / (activation scale * weight scale)
    const float* bias; const float* res; float out_scale;
    float* out; float* stats;
    int H, HW, Co, CoPad, nchunk;
    int MT, NT, linear;       // pixel tiles, channel tiles; linear = 1: plain channel-tile-major order (A/B of the XCD order)
};

__device__ __forceinline__ float small_silu(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

// T of the operand: the GroupNorm affine + SiLU on load, or nothing (an input the FIR pass has activated); out-of-image
// pixels are zeroed by a select AFTER it -- zero padding of the activated tensor, and no NaN of a clamped address leaks in.
template <bool AFFINE>
__device__ __forceinline__ float4 small_transform(float4 v, const float4& a, const float4& s, bool ok) {
    if (AFFINE) {
        v.x = small_silu(v.x * a.x + s.x); v.y = small_silu(v.y * a.y + s.y);
        v.z = small_silu(v.z * a.z + s.z); v.w = small_silu(v.w * a.w + s.w);
    }
    v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
    return v;
}

template <int BM> struct SmallGeom {
    static constexpr int W = BM == 64 ? 8 : 16;          // the image width the tile is made for
    static constexpr int R = BM / W;                     // image rows per tile
    static constexpr int SW = W + 2;
    static constexpr int SPX = (R + 2) * SW;             // staged pixels: R + 2 rows of W + 2
    static constexpr int HPL = SPX * 16, APL = SPX * 32; // bytes per channel half of a plane, per plane
    static constexpr int IMG = 2 * APL, GRP = 2 * IMG;   // one buffer (two planes); a group's two buffers
};

template <int WM, int WN, int G> constexpr int small_lds_bytes(int BM) {
    const int stage = G * (BM == 64 ? SmallGeom<64>::GRP : SmallGeom<128>::GRP);
    const int red = (G - 1) * WM * WN * 2 * 16 * 64 * 4;
    return stage > red ? stage : red;
}

// The finished tile through conv_epilogue_full's operations in its order (no output activation).  C/D map of the 32x32
// MFMA: col = lane & 31, row = (r & 3) + 8*(r >> 2) + 4*(lane >> 5).
template <bool RES, bool STATS>
__device__ __forceinline__ void small_epilogue(const SmallK& p, f32x16 (&acc)[2], int m0, int n0, int wm, int wn, int l31,
                                               int half) {
    const float ascale = p.w_hdr[0] / (p.in_bound ? bound_scale(p.in_bound[0]) : 1.0f);
    const float oscale = p.out_scale;
    const int mw = m0 + wm * 64 + 4 * half;
    const int co = n0 + wn * 32 + l31;
    const float bias = p.bias ? p.bias[co] : 0.f;
    float st_sum = 0.f, st_sq = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int mb = mw + i * 32;
        float rv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) rv[r] = 0.f;
        if (RES) {
            const float* rp = p.res + (size_t)mb * p.Co + co;
#pragma unroll
            for (int r = 0; r < 16; ++r) rv[r] = rp[(size_t)((r & 3) + 8 * (r >> 2)) * p.Co];
        }
        float* o = p.out + (size_t)mb * p.Co + co;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = (acc[i][r] * ascale + bias + rv[r]) * oscale;
            o[(size_t)((r & 3) + 8 * (r >> 2)) * p.Co] = v;
            if (STATS) { st_sum += v; st_sq += v * v; }
        }
    }
    // moments: this wave holds channel `co` of a whole 64-pixel run (lanes l and l^32 share the channel); one writer per
    // (run, channel), no atomics
    if (STATS) {
        st_sum += __shfl_xor(st_sum, 32);
        st_sq += __shfl_xor(st_sq, 32);
        if (half == 0) {
            float* sp = p.stats + ((size_t)(m0 / 64 + wm) * p.Co + co) * 2;
            sp[0] = st_sum; sp[1] = st_sq;
        }
    }
}

// G groups x (WM x WN) waves; every wave owns 64 pixels x 32 channels (two accumulator tiles).  BM = 64 * WM pixels,
// BN = 32 * WN channels.
template <int WM, int WN, int G, bool AFFINE>
__global__ __launch_bounds__(64 * WM * WN * G) void conv_small_kernel(SmallK p) {
    typedef Split<2> SP;
    typedef SP::vec vec;
    constexpr int TM = 2, BM = 64 * WM, BN = 32 * WN, RB = 32, KC = 16;
    typedef SmallGeom<BM> GE;
    constexpr int W = GE::W, R = GE::R, SW = GE::SW, HPL = GE::HPL, APL = GE::APL, IMG = GE::IMG, GRP = GE::GRP;
    constexpr int NW = WM * WN, GT = 64 * NW;            // waves / threads of a group
    constexpr int PIX = (R + 2) * W;                     // staged pixels that are loaded (the halo columns are constant zeros)
    constexpr int NU = (2 * PIX + GT - 1) / GT;          // staging units (pixel, 8-channel half) per thread
    __shared__ __attribute__((aligned(16))) char smem[small_lds_bytes<WM, WN, G>(BM)];

    // ---- which tile: the pixel tiles of a channel tile on one XCD (two where an eighth ends inside a channel tile) ----
    int nt, mt;
    {
        const int id = blockIdx.x;
        // tiles in channel-tile-major order; XCD x (workgroups go round-robin over the 8) takes the x-th eighth of that list
        const int T = p.NT * p.MT, tile = p.linear ? id : (id & 7) * ((T + 7) >> 3) + (id >> 3);
        if (tile >= T) return;                            // padding of the last eighth (whole workgroup)
        nt = tile / p.MT; mt = tile - nt * p.MT;
    }
    const int m0 = mt * BM, n0 = nt * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = wave / NW, wv = wave - g * NW;
    const int wm = wv / WN, wn = wv - wm * WN;
    const int gtid = tid - g * GT;
    const int l31 = lane & 31, half = lane >> 5;
    char* const As = smem + g * GRP;

    const int per = (p.nchunk + G - 1) / G;               // rounds: chunks of the longest group
    const int c_begin = min(p.nchunk, g * per), c_end = min(p.nchunk, c_begin + per);
    const bool busy = c_begin < c_end;                    // group-uniform

    const int bimg = m0 / p.HW;                           // the tile lies inside ONE image
    const int y0 = (m0 - bimg * p.HW) / W;
    const int Ct = p.C0 + p.C1;

    // ---- staging units of this thread: unit u = gtid + GT * k -> (staged row, column, 8-channel half) ----
    const int kh = gtid & 1;
    unsigned goff0[NU], goff1[NU];
    int slds[NU];
    bool sval[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) {
        int pp = (gtid + GT * k) >> 1;
        if (pp >= PIX) pp = gtid >> 1;                    // surplus unit: repeats unit 0 -- the same bytes to the same place
        const int sr = pp / W, x = pp - sr * W;
        const int y = y0 + sr - 1;
        sval[k] = y >= 0 && y < p.H;
        const unsigned pix = (unsigned)((bimg * p.H + (sval[k] ? y : 0)) * W + x);        // row 0 of the image: always legal
        goff0[k] = (pix * (unsigned)p.C0 + 8u * kh) * 4u;
        goff1[k] = (pix * (unsigned)p.C1 + 8u * kh) * 4u;
        slds[k] = kh * HPL + (sr * SW + x + 1) * 16;
    }
    // ---- A fragments: output pixel ml of the tile at tap (ty, tx) sits at staged pixel (r + ty) * SW + x + tx ----
    int abase[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int ml = wm * 64 + i * 32 + l31;
        const int r = ml / W, x = ml - r * W;
        abase[i] = half * HPL + (r * SW + x) * 16;
    }
    // ---- B fragment: 16 bytes per lane of the packed weights (halves pre-swizzled by the pack) ----
    const unsigned planeB = (unsigned)p.CoPad * RB;
    const unsigned slab = 2u * planeB;
    const unsigned w_tap = (unsigned)p.nchunk * slab;
    const char* const wlane = p.w + (unsigned)(n0 + wn * 32 + l31) * RB + 16u * (unsigned)(half ^ ((l31 >> 3) & 1));
    auto load_b = [&](vec (&bb)[2], int c, int t) {
        const char* wt = wlane + ((unsigned)t * w_tap + (unsigned)c * slab);
        bb[0] = *reinterpret_cast<const vec*>(wt);
        bb[1] = *reinterpret_cast<const vec*>(wt + planeB);
    };

    const float xscale = F16_ACT_SCALE * (p.in_bound ? bound_scale(p.in_bound[0]) : 1.0f);
    float4 xr[NU][2], ca[2], cs[2];
    auto stage_load = [&](int c) {                        // activations (and GroupNorm coefficients) of chunk c -> registers
        const int cc = c * KC;
        const bool first = cc < p.C0;                     // wave-uniform: a chunk lies inside one source
        const char* src = reinterpret_cast<const char*>(first ? p.src0 : p.src1);
        const unsigned cb = (unsigned)(first ? cc : cc - p.C0) * 4u;
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            const unsigned o = (first ? goff0[k] : goff1[k]) + cb;
            xr[k][0] = *reinterpret_cast<const float4*>(src + o);
            xr[k][1] = *reinterpret_cast<const float4*>(src + o + 16);
        }
        if (AFFINE) {
            const size_t co = (size_t)bimg * Ct + cc + 8 * kh;
            ca[0] = *reinterpret_cast<const float4*>(p.coef_a + co);
            ca[1] = *reinterpret_cast<const float4*>(p.coef_a + co + 4);
            cs[0] = *reinterpret_cast<const float4*>(p.coef_s + co);
            cs[1] = *reinterpret_cast<const float4*>(p.coef_s + co + 4);
        }
    };
    auto stage_store = [&](int buf) {                     // transform + split + LDS write of the registers above
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            vec pl[2];
            SP::split(small_transform<AFFINE>(xr[k][0], ca[0], cs[0], sval[k]),
                      small_transform<AFFINE>(xr[k][1], ca[1], cs[1], sval[k]), xscale, pl);
            char* A = As + buf * IMG + slds[k];
            *reinterpret_cast<vec*>(A) = pl[0];
            *reinterpret_cast<vec*>(A + APL) = pl[1];
        }
    };
    vec a[2][TM][2];
    auto read_a = [&](vec (&aa)[TM][2], const char* img, int t) {       // both planes of both pixel blocks at tap t
        const int toff = ((t / 3) * SW + (t % 3)) * 16;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            aa[i][0] = *reinterpret_cast<const vec*>(img + abase[i] + toff);
            aa[i][1] = *reinterpret_cast<const vec*>(img + APL + abase[i] + toff);
        }
    };

    f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    // ---- prologue: the first chunk's operands are requested before anything waits ----
    vec b[3][2];
    if (busy) {
        stage_load(c_begin);
        load_b(b[0], c_begin, 0);
        load_b(b[1], c_begin, 1);
    }
    // the halo columns of this group's two images (left / right of every staged row, both planes, both halves): nothing else
    // ever writes them; every other staged pixel is rewritten by each chunk's staging
    for (int u = gtid; u < 2 * (R + 2) * 8; u += GT) {
        const int ph = u & 3, side = (u >> 2) & 1, q = u >> 3;
        const int buf = q / (R + 2), row = q - buf * (R + 2);
        const int spx = row * SW + (side ? W + 1 : 0);
        *reinterpret_cast<float4*>(As + buf * IMG + (ph >> 1) * APL + (ph & 1) * HPL + spx * 16) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (busy) stage_store(0);
    __syncthreads();

    for (int it = 0; it < per; ++it) {
        const int c = c_begin + it;
        if (c < c_end) {                                   // group-uniform; an idle group only keeps the barrier count
            const int cn = min(c + 1, c_end - 1);          // the last chunk re-fetches itself: no load behind a branch
            stage_load(cn);
            const char* img = As + (it & 1) * IMG;
            read_a(a[0], img, 0);
            __builtin_amdgcn_sched_barrier(0);             // (the scheduler would otherwise sink the prefetches to their uses)
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                if (t < 8) read_a(a[(t + 1) & 1], img, t + 1);
                if (t < 7) load_b(b[(t + 2) % 3], c, t + 2);              // two K-steps ahead; the set tap t - 1 has freed
                else load_b(b[(t + 2) % 3], cn, t - 7);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < SP::NTERM; ++q)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
                        acc[i] = SP::mfma(a[t & 1][i][SP::qa(q)], b[t % 3][SP::qb(q)], acc[i]);
                __builtin_amdgcn_sched_barrier(0);
                if (t == 3) {                              // next chunk's image into the idle buffer, behind four taps of MFMAs
                    stage_store((it & 1) ^ 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __syncthreads();
    }

    // ---- reduction over the K groups, in group order ----
    float* const red = reinterpret_cast<float*>(smem);     // every image has been read: the last barrier is behind us
    if (g > 0) {
        float* o = red + (size_t)((g - 1) * NW + wv) * (TM * 16 * 64) + lane;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[(i * 16 + r) * 64] = acc[i][r];
    }
    __syncthreads();
    if (g > 0) return;
#pragma unroll 1
    for (int gg = 1; gg < G; ++gg) {
        const float* o = red + (size_t)((gg - 1) * NW + wv) * (TM * 16 * 64) + lane;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] += o[(i * 16 + r) * 64];
    }
    if (p.res) {
        if (p.stats) small_epilogue<true, true>(p, acc, m0, n0, wm, wn, l31, half);
        else small_epilogue<true, false>(p, acc, m0, n0, wm, wn, l31, half);
    } else {
        if (p.stats) small_epilogue<false, true>(p, acc, m0, n0, wm, wn, l31, half);
        else small_epilogue<false, false>(p, acc, m0, n0, wm, wn, l31, half);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------

// The kernel instances: (image width, WM, WN, G).  evc_small_conv_args::variant names one (1-based), + 16 = linear order.
struct SmallVariant { int W, wm, wn, g; };
constexpr SmallVariant SMALL_VARIANTS[4] = {
    {8, 1, 1, 8},       // 1:  64 pixels x 32 channels, 8 K groups
    {8, 1, 2, 4},       // 2:  64 x 64, 4 K groups
    {16, 2, 1, 4},      // 3: 128 x 32, 4 K groups
    {16, 2, 2, 2},      // 4: 128 x 64, 2 K groups
};

struct SmallLaunch {
    int variant;        // 1-based index into SMALL_VARIANTS
    bool affine;
    dim3 grid;
    int threads;
    SmallK k;
};

int small_resolve(const evc_small_conv_args* a, SmallLaunch& p) {
    if (!a || !a->src0 || !a->w_packed || !a->out) return EVC_EINVAL;
    if (a->B <= 0 || a->H <= 0 || a->W <= 0 || a->C0 <= 0 || a->C1 < 0 || a->Co <= 0) return EVC_EINVAL;
    if ((a->C1 > 0) != (a->src1 != nullptr)) return EVC_EINVAL;
    if ((a->coef_a != nullptr) != (a->coef_s != nullptr)) return EVC_EINVAL;
    if (a->arith != EVC_ARITH_F16X3) return EVC_EUNSUPPORTED;
    if (a->KH != 3 || a->KW != 3) return EVC_EUNSUPPORTED;
    if (a->H != a->W || (a->H != 8 && a->H != 16)) return EVC_EUNSUPPORTED;
    if (a->invariant || a->x2_w_packed) return EVC_EUNSUPPORTED;
    if (a->act_out != EVC_ACT_NONE) return EVC_EUNSUPPORTED;
    if (a->coef_a ? a->act_in != EVC_ACT_SILU : a->act_in != EVC_ACT_NONE) return EVC_EUNSUPPORTED;   // MODE_AFFINE_SILU / MODE_PLAIN
    if (a->C0 % 16 != 0 || a->C1 % 16 != 0 || a->Co % 32 != 0) return EVC_EUNSUPPORTED;
    const long long HW = (long long)a->H * a->W, M = HW * a->B, Ct = (long long)a->C0 + a->C1;
    if (M * (a->C0 > a->C1 ? a->C0 : a->C1) * 4 >= (1LL << 32) || M * a->Co >= (1LL << 31)) return EVC_EUNSUPPORTED;
    if (9 * Ct * 2 * evc_conv_co_pad(a->Co) * 2 >= (1LL << 32)) return EVC_EUNSUPPORTED;
    const int v = a->variant & 15;
    if ((a->variant & ~31) != 0 || v > 4) return EVC_EUNSUPPORTED;
    if (v) p.variant = v;
    else {
        // Measured per shape at B = 1, 6 and 9 (profiles/NOTES.md "Small-grid convolutions", profiles/r07_small_conv_ab*.log): a
        // workgroup's time hardly depends on the batch, so the kernel wins where its workgroups come close to filling the chip
        // once, or where K is short enough that the convolution's split-K overheads dominate whatever the grid.
        const long long cus = 256;
        if (a->H == 8) {
            // up to 768 input channels: faster at every batch measured.  The concat layers (1344 / 1536 channels): faster at
            // B = 9 (216 workgroups), slower at B = 6 (144) and 1 -- taken where the last round of workgroups is 3/4 full.
            const long long T = (long long)(a->Co / 32) * a->B, rounds = (T + cus - 1) / cus;
            if (Ct > 768 && 4 * T < 3 * rounds * cus) return EVC_EUNSUPPORTED;
            p.variant = 1;
        } else {
            // 16 x 16: only the short K ranges (up to 384 input channels), on 128 x 32 tiles, while those fit one round: 25.9 us
            // against 32.5 at 384 -> 384, B = 9 (216 workgroups); 28.0 against 33.2 at 384 -> 576, B = 6 (216).  At B = 9 that
            // layer has 324 such tiles (52 us) and its 128 x 64 tiles are within the convolution's spread (42.6 against 43.7): left
            // to the convolution.  From 576 channels on its split-K plan runs at 250 .. 320 TFLOP/s and keeps its layers.
            if (Ct > 384 || (long long)(a->Co / 32) * 2 * a->B > cus) return EVC_EUNSUPPORTED;
            p.variant = 3;
        }
    }
    const SmallVariant& sv = SMALL_VARIANTS[p.variant - 1];
    if (sv.W != a->W || a->Co % (32 * sv.wn) != 0) return EVC_EUNSUPPORTED;
    p.affine = a->coef_a != nullptr;
    p.threads = 64 * sv.wm * sv.wn * sv.g;
    SmallK& k = p.k;
    k.C0 = a->C0; k.C1 = a->C1; k.H = a->H; k.HW = (int)HW; k.Co = a->Co; k.CoPad = evc_conv_co_pad(a->Co);
    k.nchunk = (int)(Ct / 16);
    k.MT = (int)(M / (64 * sv.wm)); k.NT = a->Co / (32 * sv.wn); k.linear = (a->variant >> 4) & 1;
    p.grid = dim3((unsigned)(k.linear ? k.NT * k.MT : (k.NT * k.MT + 7) / 8 * 8));
    return EVC_OK;
}

int small_kernel_name(const SmallLaunch& p, char* buf, int n) {
    const SmallVariant& sv = SMALL_VARIANTS[p.variant - 1];
    return snprintf(buf, n, "conv_small_kernel<%d, %d, %d, %s>", sv.wm, sv.wn, sv.g, p.affine ? "true" : "false");
}

template <int WM, int WN, int G>
void small_launch(const SmallLaunch& p, hipStream_t st) {
    if (p.affine) hipLaunchKernelGGL((conv_small_kernel<WM, WN, G, true>), p.grid, dim3(p.threads), 0, st, p.k);
    else hipLaunchKernelGGL((conv_small_kernel<WM, WN, G, false>), p.grid, dim3(p.threads), 0, st, p.k);
}

}  // namespace

extern "C" int evc_small_conv_supported(const evc_small_conv_args* a) {
    SmallLaunch p;
    return small_resolve(a, p) == EVC_OK ? 1 : 0;
}

extern "C" int evc_small_conv_plan_query(const evc_small_conv_args* a, evc_small_conv_plan* out) {
    SmallLaunch p;
    const int rc = !out ? EVC_EINVAL : small_resolve(a, p);
    if (rc != EVC_OK) return rc;
    const SmallVariant& sv = SMALL_VARIANTS[p.variant - 1];
    small_kernel_name(p, out->kernel, (int)sizeof(out->kernel));
    out->variant = p.variant; out->tile_m = 64 * sv.wm; out->tile_n = 32 * sv.wn; out->groups = sv.g;
    out->chunks = p.k.nchunk; out->rounds = (p.k.nchunk + sv.g - 1) / sv.g; out->stats_runs = p.k.HW / 64;
    return EVC_OK;
}

extern "C" int evc_small_conv_f32(const evc_small_conv_args* a, void* stream) {
    SmallLaunch p;
    const int rc = small_resolve(a, p);
    if (rc != EVC_OK) return rc;
    SmallK& k = p.k;
    k.src0 = a->src0; k.src1 = a->src1; k.coef_a = a->coef_a; k.coef_s = a->coef_s; k.in_bound = a->in_bound;
    k.w_hdr = a->w_packed;
    k.w = reinterpret_cast<const char*>(a->w_packed) + F16_HDR_BYTES;
    k.bias = a->bias; k.res = a->res; k.out_scale = a->out_scale; k.out = a->out; k.stats = a->stats_out;
    hipStream_t st = (hipStream_t)stream;
    switch (p.variant) {
        case 1: small_launch<1, 1, 8>(p, st); break;
        case 2: small_launch<1, 2, 4>(p, st); break;
        case 3: small_launch<2, 1, 4>(p, st); break;
        default: small_launch<2, 2, 2>(p, st); break;
    }
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}
