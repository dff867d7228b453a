// nin_gemm.hip -- the NIN / linear projections of the attention blocks as a plain GEMM on the fp16 matrix cores.
//
//   out[m][n] = ((sum_k T(x[m][k]) * w[n][k]) + bias[n] + res[m][n]) * out_scale        M = B*H*W pixels, K = Ci <= ~1k, N = Co
//
// Same arithmetic, to the bit, as conv_splitn_kernel<2, ...> (conv_igemm.hip) run unsplit on the 1x1 filter: the operand is
// transformed, scaled and split by split2_f16, every 16-channel K-step adds the three cross products of Split<2> in its order
// into one fp32 accumulator per output, K-steps ascend, and the epilogue is that of conv_epilogue_full.  What differs is the
// schedule, which is what those launches lacked (they are GEMMs with K of 384..768, far too short for a per-step barrier):
//   * a STAGE is 64 channels = four K-steps.  The A tile [BM][64] of a stage goes global -> registers -> transform + split ->
//     LDS planes once, double-buffered: ONE workgroup barrier per stage, 12 * TM * TN MFMAs per wave between barriers;
//   * the loads of the next stage are issued before this stage's MFMAs, unconditionally (the last stage re-fetches itself
//     into the idle buffer: no load sits behind a branch);
//   * the weights do not go through LDS -- no two waves of a workgroup column share a fragment that LDS would save a fetch
//     of, and the pack is L2-resident: a lane's B fragment (chunk c, plane q, channel n) is the 16 bytes at
//     ((c*2 + q)*CoPad + n)*32 + 16*(half ^ ((n >> 3) & 1)) of the pack, read straight into registers one stage ahead, each
//     K-step's registers refilled as soon as its MFMAs have consumed them;
//   * no K split, no workspace, no second launch, no atomics: the tile is chosen to fill the chip instead (nin_pick_tile),
//     two workgroups per CU hide the latencies.
// LDS image of one stage buffer: [4 K-steps][2 planes][BM rows][32 B]; inside a plane the 32-byte row r of K-step c sits in
// slot r ^ c and its two 16-byte halves are swapped when (r >> 3) & 1 -- the eight lanes that stage one pixel row (four
// K-steps x two halves) then hit eight distinct 16-byte slots of a 128-byte bank row (ds_write_b128 is banked in groups of
// eight lanes), and the fragment reads (ds_read_b128, row = lane & 31) keep the conflict-free pattern of conv_splitn_kernel.
//
// Replaces NIN (reference models/better/layers.py:535-544) inside AttnBlockpp (layerspp.py:230-249) in default mode.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/evc_hip.h"
#include "split_mfma.h"

namespace {

struct NinK {
    const float* x; const float* coef_a; const float* coef_s; const unsigned* in_bound;
    const char* w;            // planes of the pack (behind the header)
    const float* w_hdr;       // [0] = 1 / (activation scale * weight scale)
    const float* bias; const float* res; float out_scale;
    float* out; float* stats;
    int M, HW, K, Co, nstage;
};

// conv_epilogue_full of conv_igemm.hip for a finished (unsplit) tile without output activation: the same operations in the
// same order.  C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8*(r >> 2) + 4*(lane >> 5).
template <int TM, int TN, bool RES, bool STATS>
__device__ __forceinline__ void nin_epilogue(const NinK& p, f32x16 (&acc)[TM][TN], int m0, int n0, int wm, int wn, int l31,
                                             int half) {
    const float ascale = p.w_hdr[0] / (p.in_bound ? bound_scale(p.in_bound[0]) : 1.0f);
    const float oscale = p.out_scale;
    const int mw = m0 + wm * 32 * TM + 4 * half;
    const int cw = n0 + wn * 32 * TN + l31;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int co = cw + j * 32;
        const float bias = p.bias ? p.bias[co] : 0.f;
        float st_sum = 0.f, st_sq = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
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
                float v = (acc[i][j][r] * ascale + bias + rv[r]) * oscale;
                o[(size_t)((r & 3) + 8 * (r >> 2)) * p.Co] = v;
                if (STATS) { st_sum += v; st_sq += v * v; }
            }
        }
        // moments: this wave holds channel `co` of a whole 32*TM-pixel run (lanes l and l^32 share the channel); one
        // writer per (run, channel), no atomics
        if (STATS) {
            st_sum += __shfl_xor(st_sum, 32);
            st_sq += __shfl_xor(st_sq, 32);
            if (half == 0) {
                float* sp = p.stats + ((size_t)(m0 / (32 * TM) + wm) * p.Co + co) * 2;
                sp[0] = st_sum; sp[1] = st_sq;
            }
        }
    }
}

// An empty volatile statement that "rewrites" v: what is computed from v cannot move above it.
__device__ __forceinline__ void pin(float4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// 4 waves (2 x 2) compute a 64*TM x 64*TN tile; each wave owns 32*TM pixels x 32*TN channels.
template <int TM, int TN, bool AFFINE>
__global__ __launch_bounds__(256, 2) void nin_gemm_kernel(NinK p) {
    typedef Split<2> SP;
    typedef SP::vec vec;
    constexpr int BM = 64 * TM;
    constexpr int BN = 64 * TN;
    constexpr int RB = 32;                   // bytes per LDS / pack row: 16 fp16
    constexpr int NJ = 2 * TM;               // 8-channel pieces a thread stages per stage: BM rows x 8 pieces / 256 threads
    constexpr int PLANE = BM * RB, STEP = 2 * PLANE, BUF = 4 * STEP;
    extern __shared__ __attribute__((aligned(16))) char smem_nin[];      // [2][4][2][BM][32 B]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;
    const int m0 = blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;

    // ---- staging: thread -> piece pc (K-step sc, half skh) of rows srow + 32*j; eight threads cover a row's 256 bytes ----
    const int pc = tid & 7, sc = pc >> 1, skh = pc & 1, srow = tid >> 3;
    const char* const xg = reinterpret_cast<const char*>(p.x + (size_t)m0 * p.K) + ((size_t)srow * p.K + pc * 8) * 4;
    const unsigned xstep = 32u * (unsigned)p.K * 4u;                      // 32 rows down
    const size_t cofs = (size_t)(m0 / p.HW) * p.K + pc * 8;               // the tile lies inside one sample
    int a_wr[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int row = srow + 32 * j;
        a_wr[j] = sc * STEP + (row ^ sc) * RB + 16 * (skh ^ ((row >> 3) & 1));
    }
    // fragment reads: row l31 of the wave's i-th 32-row block, K-step c in slot row ^ c
    const int swz = 16 * (half ^ ((l31 >> 3) & 1));
    const int a_rd = wm * 32 * TM * RB + swz;
    const char* const wg = p.w + (size_t)(n0 + wn * 32 * TN + l31) * RB + swz;
    const unsigned wplane = (unsigned)p.Co * RB;                          // Co % 64 == 0: the pack has no padded rows

    const float xscale = F16_ACT_SCALE * (p.in_bound ? bound_scale(p.in_bound[0]) : 1.0f);

    float4 areg[NJ][2], ca[2], cs[2];
    vec breg[4][TN][2];
    auto load_a = [&](int s) {
        const char* src = xg + (size_t)s * 256;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            areg[j][0] = *reinterpret_cast<const float4*>(src + j * xstep);
            areg[j][1] = *reinterpret_cast<const float4*>(src + j * xstep + 16);
        }
        if (AFFINE) {
            const float* a = p.coef_a + cofs + s * 64;
            const float* c = p.coef_s + cofs + s * 64;
            ca[0] = *reinterpret_cast<const float4*>(a); ca[1] = *reinterpret_cast<const float4*>(a + 4);
            cs[0] = *reinterpret_cast<const float4*>(c); cs[1] = *reinterpret_cast<const float4*>(c + 4);
        }
    };
    auto load_b = [&](int s, int c) {
        const char* src = wg + (size_t)(s * 4 + c) * 2 * wplane;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 2; ++q) breg[c][j][q] = *reinterpret_cast<const vec*>(src + q * wplane + j * 32 * RB);
    };
    auto affine = [&](float4 v, const float4& a, const float4& s) {
        if (AFFINE) { v.x = v.x * a.x + s.x; v.y = v.y * a.y + s.y; v.z = v.z * a.z + s.z; v.w = v.w * a.w + s.w; }
        return v;
    };
    auto store_a = [&](int buf) {
        char* A = smem_nin + buf * BUF;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            vec pl[2];
            pin(areg[j][0]); pin(areg[j][1]);          // the transform stays HERE: hoisted to the loads it would wait for them
            SP::split(affine(areg[j][0], ca[0], cs[0]), affine(areg[j][1], ca[1], cs[1]), xscale, pl);
            *reinterpret_cast<vec*>(A + a_wr[j]) = pl[0];
            *reinterpret_cast<vec*>(A + a_wr[j] + PLANE) = pl[1];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load_a(0);
#pragma unroll
    for (int c = 0; c < 4; ++c) load_b(0, c);
    store_a(0);
    __syncthreads();

    for (int s = 0; s < p.nstage; ++s) {
        const int buf = s & 1;
        const int sn = min(s + 1, p.nstage - 1);       // the last stage re-fetches itself: no load behind a branch
        load_a(sn);
        __builtin_amdgcn_sched_barrier(0);             // (the scheduler would otherwise sink the prefetches to their uses)
        const char* Ab = smem_nin + buf * BUF + a_rd;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            vec a[TM][2];
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    a[i][q] = *reinterpret_cast<const vec*>(Ab + c * STEP + q * PLANE + ((i * 32 + l31) ^ c) * RB);
#pragma unroll
            for (int t = 0; t < SP::NTERM; ++t)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = SP::mfma(a[i][SP::qa(t)], breg[c][j][SP::qb(t)], acc[i][j]);
            __builtin_amdgcn_sched_barrier(0);
            load_b(sn, c);                             // this K-step's weight registers are free again: refill them
            __builtin_amdgcn_sched_barrier(0);
            if (c == 1) store_a(buf ^ 1);              // next stage's A (fetched at the top) into the idle buffer, among the
                                                       // MFMAs of the third K-step
        }
        __syncthreads();
    }

    if (p.res) {
        if (p.stats) nin_epilogue<TM, TN, true, true>(p, acc, m0, n0, wm, wn, l31, half);
        else nin_epilogue<TM, TN, true, false>(p, acc, m0, n0, wm, wn, l31, half);
    } else {
        if (p.stats) nin_epilogue<TM, TN, false, true>(p, acc, m0, n0, wm, wn, l31, half);
        else nin_epilogue<TM, TN, false, false>(p, acc, m0, n0, wm, wn, l31, half);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------

constexpr int NIN_SLOTS = 512;      // workgroups resident at once: 256 CUs x 2 (__launch_bounds__(256, 2), <= 64 KB LDS each)

constexpr int NIN_CONV_KEEPS = 256;  // grids of this many 128 x 192 convolution tiles stay on the convolution (nin_resolve)

struct NinLaunch {
    int tm, tn, runs;
    bool affine;
    dim3 grid;
    size_t lds;
    NinK k;
};

// THE tile choice: a pure function of (M, K, N) and the pixels per sample.  Candidates are the tiles that divide H*W (no tile
// straddles two samples) and N; each is charged rounds-of-resident-workgroups x (tile area + a fixed per-workgroup part worth
// a 64 x 64 tile: prologue, epilogue, barriers), the cheapest wins, the larger tile on a tie.  K only scales every candidate
// alike.
bool nin_pick_tile(long long M, int K, int N, int HW, int& tm, int& tn) {
    (void)K;
    static const int cand[3][2] = {{2, 2}, {2, 1}, {1, 1}};
    long long best = -1;
    for (const auto& c : cand) {
        const int bm = 64 * c[0], bn = 64 * c[1];
        if (HW % bm != 0 || N % bn != 0) continue;
        const long long wgs = (M / bm) * (N / bn);
        const long long cost = ((wgs + NIN_SLOTS - 1) / NIN_SLOTS) * (bm * bn + 64 * 64);
        if (best < 0 || cost < best) { best = cost; tm = c[0]; tn = c[1]; }
    }
    return best >= 0;
}

int nin_resolve(const evc_nin_args* a, NinLaunch& p) {
    if (!a || !a->x || !a->w_packed || !a->out) return EVC_EINVAL;
    if (a->B <= 0 || a->H <= 0 || a->W <= 0 || a->Ci <= 0 || a->Co <= 0) return EVC_EINVAL;
    if (a->arith != EVC_ARITH_F16X3) return EVC_EUNSUPPORTED;
    if (a->x1) return EVC_EUNSUPPORTED;
    if (a->Ci % 64 != 0 || a->Co % 64 != 0) return EVC_EUNSUPPORTED;
    if (a->act_out != EVC_ACT_NONE) return EVC_EUNSUPPORTED;
    const bool coef = a->coef_a && a->coef_s;
    if ((a->coef_a != nullptr) != (a->coef_s != nullptr)) return EVC_EINVAL;
    if (coef == (a->in_bound != nullptr)) return EVC_EUNSUPPORTED;       // exactly one of the two on-load forms
    const long long HW = (long long)a->H * a->W, M = HW * a->B;
    if (M * a->Ci * 4 >= (1LL << 32) || M * a->Co >= (1LL << 31) || HW >= (1LL << 31)) return EVC_EUNSUPPORTED;
    if (a->tile) {
        p.tm = a->tile / 10; p.tn = a->tile % 10;
        if ((a->tile != 22 && a->tile != 21 && a->tile != 11) || HW % (64 * p.tm) != 0 || a->Co % (64 * p.tn) != 0) return EVC_EUNSUPPORTED;
    } else {
        // Measured (profiles/NOTES.md): where the convolution's own 128 x 192 tiles fill the chip unsplit (at least one per CU)
        // its kernel is the faster one -- B = 9, 32 x 32 q | k | v: 35.4 us against 37.1 -- so those grids stay with it.
        if (a->Co % 192 == 0 && HW % 128 == 0 && (M / 128) * (a->Co / 192) >= NIN_CONV_KEEPS) return EVC_EUNSUPPORTED;
        if (!nin_pick_tile(M, a->Ci, a->Co, (int)HW, p.tm, p.tn)) return EVC_EUNSUPPORTED;
    }
    p.affine = coef;
    p.runs = (int)HW / (32 * p.tm);
    p.grid = dim3((unsigned)(M / (64 * p.tm)), (unsigned)(a->Co / (64 * p.tn)));
    p.lds = (size_t)2 * 4 * 2 * 64 * p.tm * 32;
    NinK& k = p.k;
    k.M = (int)M; k.HW = (int)HW; k.K = a->Ci; k.Co = a->Co; k.nstage = a->Ci / 64;
    return EVC_OK;
}

int nin_kernel_name(const NinLaunch& p, char* buf, int n) {
    return snprintf(buf, n, "nin_gemm_kernel<%d, %d, %s>", p.tm, p.tn, p.affine ? "true" : "false");
}

template <int TM, int TN>
void nin_launch(const NinLaunch& p, hipStream_t st) {
    if (p.affine) hipLaunchKernelGGL((nin_gemm_kernel<TM, TN, true>), p.grid, dim3(256), p.lds, st, p.k);
    else hipLaunchKernelGGL((nin_gemm_kernel<TM, TN, false>), p.grid, dim3(256), p.lds, st, p.k);
}

}  // namespace

extern "C" int evc_nin_gemm_supported(const evc_nin_args* a) {
    NinLaunch p;
    return nin_resolve(a, p) == EVC_OK ? 1 : 0;
}

extern "C" int evc_nin_gemm_plan_query(const evc_nin_args* a, evc_nin_plan* out) {
    NinLaunch p;
    const int rc = !out ? EVC_EINVAL : nin_resolve(a, p);
    if (rc != EVC_OK) return rc;
    nin_kernel_name(p, out->kernel, (int)sizeof(out->kernel));
    out->tile_m = 64 * p.tm; out->tile_n = 64 * p.tn; out->stages = p.k.nstage; out->stats_runs = p.runs;
    return EVC_OK;
}

extern "C" int evc_nin_gemm_f32(const evc_nin_args* a, void* stream) {
    NinLaunch p;
    const int rc = nin_resolve(a, p);
    if (rc != EVC_OK) return rc;
    NinK& k = p.k;
    k.x = a->x; k.coef_a = a->coef_a; k.coef_s = a->coef_s; k.in_bound = a->in_bound;
    k.w_hdr = a->w_packed;
    k.w = reinterpret_cast<const char*>(a->w_packed) + F16_HDR_BYTES;
    k.bias = a->bias; k.res = a->res; k.out_scale = a->out_scale; k.out = a->out; k.stats = a->stats_out;
    hipStream_t st = (hipStream_t)stream;
    if (p.tm == 2 && p.tn == 2) nin_launch<2, 2>(p, st);
    else if (p.tm == 2) nin_launch<2, 1>(p, st);
    else nin_launch<1, 1>(p, st);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}
