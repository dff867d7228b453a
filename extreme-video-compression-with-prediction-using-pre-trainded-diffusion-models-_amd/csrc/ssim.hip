// ssim.hip -- the structural similarity of the reference's metric helpers (fvd_utils/calculate_ssim.py:6-23), one value per
// plane: the 11x11 Gaussian window over the VALID region of mu1, mu2, E[x1^2], E[x2^2], E[x1 x2], the SSIM map from them and
// the map's mean.
//
// Everything is float64, as the reference's numpy is: sigma^2 = E[x^2] - mu^2 is taken against C2 = 9e-4, and an fp32
// evaluation is wrong in the fourth digit on nearly flat content.  The fp32 inputs are widened on the way in; their pairwise
// products are then exact in double, so the only roundings are the tap-weighted sums and the map itself.
//
// One workgroup per 16x16 tile of the map.  It stages the 26x26 halo tile of both planes in LDS once (as fp32: the widening
// is exact), filters the five quantities along rows into LDS (26 rows x 16 columns, double), then along columns in
// registers, evaluates the map and reduces its tile.  The five filtered maps never go to memory.
//
// Sums are deterministic and batch-invariant: a tile's 256 values go through a wave shuffle tree and a fixed-order pass over
// the four wave totals; the tile total leaves with a plain store into the workspace; a second launch, one workgroup per
// plane, adds the plane's tile totals in an order that depends on (H, W) only.  No atomics, and nothing a plane's value
// could learn from N or from its neighbours.
//
// Nothing is clamped: a NaN or an infinity makes every window that holds it NaN (inf - inf for an infinity), hence the
// plane's mean, as the formula does.  Lanes outside the map are dropped by a select, never by a multiplication.
#include <hip/hip_runtime.h>
#include "../../include/evc_hip.h"

// The map is evaluated operation by operation, as numpy does: a contracted mu1*mu1 + mu2*mu2 would no longer equal
// 2 * mu1*mu2 on identical planes, and SSIM(x, x) would miss 1.0 by an ulp.  The filter sums ask for fma() by name.
#pragma clang fp contract(off)

namespace {

constexpr int SSIM_THREADS = 256;
constexpr int SSIM_WAVES = SSIM_THREADS / 64;
constexpr int WIN = 11;                      // window taps per axis
constexpr int TILE = 16;                     // map tile: TILE x TILE values, one per thread
constexpr int HALO = TILE + WIN - 1;         // 26 input rows / columns per tile
constexpr int IN_LD = 48;                    // fp32 row stride of the staged inputs: 16 mod 32, so the two rows that one
                                             // 32-lane group of the row pass reads fall on disjoint banks
constexpr long long MAX_BLOCKS = 1LL << 30;  // per launch
#define EVC_LAUNCH_OK() (hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH)

// total of v over the workgroup, valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* wave_total) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = wave_total[0];
    for (int w = 1; w < SSIM_WAVES; ++w) s += wave_total[w];
    return s;
}

__global__ void __launch_bounds__(SSIM_THREADS)
ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, long long plane0, int H, int W, int tiles_x,
                 int tiles, const double* __restrict__ taps11, double c1, double c2, double* __restrict__ partial) {
    __shared__ float in_a[HALO * IN_LD];
    __shared__ float in_b[HALO * IN_LD];
    __shared__ double rowf[5][HALO * TILE];
    __shared__ double tap[WIN];
    __shared__ double wave_total[SSIM_WAVES];
    const int tid = threadIdx.x;
    const long long plane = plane0 + (long long)blockIdx.x / tiles;
    const int tile = (int)((long long)blockIdx.x % tiles);
    const int y0 = (tile / tiles_x) * TILE, x0 = (tile % tiles_x) * TILE;    // map (y, x) reads inputs (y .. y+10, x .. x+10)
    const long long base = plane * H * W;

    if (tid < WIN) tap[tid] = taps11[tid];
    for (int i = tid; i < HALO * HALO; i += SSIM_THREADS) {
        const int r = i / HALO, c = i % HALO;
        const int gy = y0 + r, gx = x0 + c;
        const bool inside = gy < H && gx < W;                 // beyond the plane: zeros, read by dropped lanes only
        const long long at = base + (long long)gy * W + gx;
        in_a[r * IN_LD + c] = inside ? a[at] : 0.0f;
        in_b[r * IN_LD + c] = inside ? b[at] : 0.0f;
    }
    __syncthreads();

    // along rows: HALO x TILE values of each quantity
    for (int i = tid; i < HALO * TILE; i += SSIM_THREADS) {
        const int r = i / TILE, c = i % TILE;
        const float* pa = in_a + r * IN_LD + c;
        const float* pb = in_b + r * IN_LD + c;
        double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const double t = tap[k], x1 = (double)pa[k], x2 = (double)pb[k];
            m1 = fma(t, x1, m1);
            m2 = fma(t, x2, m2);
            s11 = fma(t, x1 * x1, s11);          // products of two widened floats: exact
            s22 = fma(t, x2 * x2, s22);
            s12 = fma(t, x1 * x2, s12);
        }
        rowf[0][i] = m1; rowf[1][i] = m2; rowf[2][i] = s11; rowf[3][i] = s22; rowf[4][i] = s12;
    }
    __syncthreads();

    // along columns, the map, the tile's sum
    const int y = tid / TILE, x = tid % TILE;
    double mu1 = 0.0, mu2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
    for (int k = 0; k < WIN; ++k) {
        const double t = tap[k];
        const int at = (y + k) * TILE + x;
        mu1 = fma(t, rowf[0][at], mu1);
        mu2 = fma(t, rowf[1][at], mu2);
        e11 = fma(t, rowf[2][at], e11);
        e22 = fma(t, rowf[3][at], e22);
        e12 = fma(t, rowf[4][at], e12);
    }
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const double sigma1_sq = e11 - mu1_sq, sigma2_sq = e22 - mu2_sq, sigma12 = e12 - mu1_mu2;
    const double value = ((2.0 * mu1_mu2 + c1) * (2.0 * sigma12 + c2)) /
                         ((mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2));
    const bool in_map = y0 + y < H - (WIN - 1) && x0 + x < W - (WIN - 1);
    const double total = block_sum(in_map ? value : 0.0, wave_total);
    if (tid == 0) partial[plane * tiles + tile] = total;
}

// out[plane] = (sum of the plane's tile totals) / (number of map values): lane t takes tiles t, t + 256, ... in that order
__global__ void __launch_bounds__(SSIM_THREADS)
ssim_finish_kernel(const double* __restrict__ partial, long long plane0, int tiles, double count, double* __restrict__ out) {
    __shared__ double wave_total[SSIM_WAVES];
    const long long plane = plane0 + blockIdx.x;
    const double* p = partial + plane * tiles;
    double acc = 0.0;
    for (int i = threadIdx.x; i < tiles; i += SSIM_THREADS) acc += p[i];
    const double total = block_sum(acc, wave_total);
    if (threadIdx.x == 0) out[plane] = total / count;
}

__host__ long long tiles_of(int H, int W, int* tiles_x) {
    const long long tx = ((long long)W - (WIN - 1) + TILE - 1) / TILE, ty = ((long long)H - (WIN - 1) + TILE - 1) / TILE;
    if (tiles_x) *tiles_x = (int)tx;
    return tx * ty;
}

}  // namespace

extern "C" long long evc_ssim_workspace_bytes(int N, int H, int W) {
    if (N < 0 || H < WIN || W < WIN) return EVC_EINVAL;
    const long long tiles = tiles_of(H, W, nullptr);
    if (tiles > MAX_BLOCKS) return EVC_EUNSUPPORTED;
    return (long long)N * tiles * (long long)sizeof(double);
}

extern "C" int evc_ssim_planes_f32(const float* a, const float* b, int N, int H, int W, const double* taps11, double c1,
                                   double c2, double* out, void* ws, void* stream) {
    if (N < 0 || H < WIN || W < WIN) return EVC_EINVAL;
    if (N == 0) return EVC_OK;
    if (!a || !b || !taps11 || !out || !ws) return EVC_EINVAL;
    int tiles_x = 0;
    const long long tiles = tiles_of(H, W, &tiles_x);
    if (tiles > MAX_BLOCKS) return EVC_EUNSUPPORTED;
    const double count = (double)((long long)(H - (WIN - 1)) * (W - (WIN - 1)));
    const long long per_launch = MAX_BLOCKS / tiles;          // planes per launch: a plane's value does not depend on it
    for (long long p0 = 0; p0 < N; p0 += per_launch) {
        const long long n = N - p0 < per_launch ? N - p0 : per_launch;
        hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)(n * tiles)), dim3(SSIM_THREADS), 0, (hipStream_t)stream, a, b, p0, H,
                           W, tiles_x, (int)tiles, taps11, c1, c2, (double*)ws);
        hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)n), dim3(SSIM_THREADS), 0, (hipStream_t)stream,
                           (const double*)ws, p0, (int)tiles, count, out);
    }
    return EVC_LAUNCH_OK();
}
