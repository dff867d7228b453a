// msssim.hip -- the levels of multi-scale SSIM as pytorch_msssim.ms_ssim defines them (win_size 11, sigma 1.5, the valid region
// only): per pair of planes and per level the mean of the SSIM map and the mean of its contrast-structure factor
//     cs   = (2 s12 + c2) / (s1 + s2 + c2)
//     ssim = ((2 mu1 mu2 + c1) / (mu1^2 + mu2^2 + c1)) * cs,          s = E[.] - mu mu,
// over a pyramid whose level l + 1 is the 2x2 mean of level l (avg_pool2d(kernel 2, stride 2, padding = size % 2),
// count_include_pad: an odd axis gets one zero row / column in front, the divisor is always 4).  The host combines a plane's
// 2 x levels numbers into the value (msssim.py): no pow on the device.
//
// Everything is float64, as in ssim.hip.  Level 0 reads the fp32 planes and widens them; the pool kernel writes levels >= 1 as
// float64 into the workspace, 0.25 * ((x00 + x01) + (x10 + x11)).  The tile kernel then does for every level of every plane
// what ssim_tile_kernel does -- the 26x26 halo of both planes staged once in LDS, the five quantities filtered along rows into
// LDS and along columns in registers, both maps evaluated, two tile sums reduced by a shuffle tree and a fixed pass over the
// four wave totals, stored plainly -- in two launches, one per input type: level 0 from fp32 with ssim_tile_kernel's LDS
// footprint and occupancy, and all levels above from float64 in one launch, where a workgroup finds its (plane, level, tile)
// from a by-value table of the levels' sizes and offsets.  (One launch for all levels has to reserve the float64 staging for
// the fp32 tiles too, 4 workgroups per CU instead of 6: 5.54 ms of tile work against 4.75 ms for 90 planes of 1920x1080;
// profiles/NOTES.md.)  A last launch,
// one workgroup per (plane, level), adds that level's tile totals in an order fixed by the level's size and divides by the
// map's size.  levels - 1 pool launches + 3: seven for five levels, whatever N is (beyond 2^30 workgroups a launch is cut by
// planes, which no plane's value can see).
//
// No atomics; a plane's numbers depend on its own samples and (H, W, levels) only.  Nothing is clamped: a NaN or an infinity
// makes every window that holds it NaN at every level that sees it, and stays in its plane.  Lanes outside a map are dropped
// by a select.
#include <hip/hip_runtime.h>
#include "../../include/evc_hip.h"

// The maps are evaluated operation by operation: on identical planes 2 * s12 and s1 + s2, 2 * mu1 mu2 and mu1^2 + mu2^2 are
// then the same doubles and every level is exactly 1.0.  The filter sums ask for fma() by name.
#pragma clang fp contract(off)

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_WAVES = MS_THREADS / 64;
constexpr int WIN = 11;                      // window taps per axis
constexpr int TILE = 16;                     // map tile: TILE x TILE values, one per thread
constexpr int HALO = TILE + WIN - 1;         // 26 input rows / columns per tile
// Row stride of the staged inputs, in elements, for both element widths.  A 32-lane group of the row pass reads two rows of
// 16 adjacent elements.  fp32 (ds_read_b32, bank = dword mod 32): 48 = 16 mod 32, so the second row starts 16 banks after the
// first and the two rows fill the 32 banks once.  fp64 (ds_read_b64, bank = dword mod 64, two banks per lane): 48 doubles =
// 96 dwords = 32 mod 64, so the rows take banks b .. b+31 and b+32 .. b+63.  The filtered rows (TILE doubles per row, rows
// adjacent) are read by the column pass as 32 adjacent doubles per group: all 64 banks once.
constexpr int IN_LD = 48;
constexpr int MAX_LEVELS = 8;
constexpr int POOL_OUTS = 2;                 // adjacent outputs of one row per thread of the pool kernel
constexpr long long MAX_BLOCKS = 1LL << 30;  // per launch
#define EVC_LAUNCH_OK() (hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH)

// The pyramid of one call, by value.  Levels >= 1 of a plane lie one after the other in the workspace (pyr_off[l] doubles from
// the plane's start, pyr_plane doubles per plane); a plane's tiles are numbered level by level (tile_end[l]: one past the last
// tile of level l).
struct Pyramid {
    int levels;
    int H[MAX_LEVELS], W[MAX_LEVELS], tiles_x[MAX_LEVELS], tile_end[MAX_LEVELS];
    long long pyr_off[MAX_LEVELS];
    long long pyr_plane;
};

// totals of v0 and of v1 over the workgroup, valid in thread 0
__device__ __forceinline__ void block_sum2(double& v0, double& v1, double (*wave_total)[MS_WAVES]) {
    for (int off = 32; off > 0; off >>= 1) {
        v0 += __shfl_down(v0, off, 64);
        v1 += __shfl_down(v1, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        wave_total[0][threadIdx.x >> 6] = v0;
        wave_total[1][threadIdx.x >> 6] = v1;
    }
    __syncthreads();
    v0 = wave_total[0][0];
    v1 = wave_total[1][0];
    for (int w = 1; w < MS_WAVES; ++w) {
        v0 += wave_total[0][w];
        v1 += wave_total[1][w];
    }
}

// p[0 .. 3] widened; 16-byte loads where the address allows
__device__ __forceinline__ void load4(const float* p, double v[4]) {
    if (((unsigned long long)p & 15) == 0) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
}
__device__ __forceinline__ void load4(const double* p, double v[4]) {
    if (((unsigned long long)p & 15) == 0) {
        const double2 lo = *reinterpret_cast<const double2*>(p), hi = *reinterpret_cast<const double2*>(p + 2);
        v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
    } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
}

// Level l -> l + 1 of both planes' pyramids (blockIdx.y: 0 the a side, 1 the b side).  A thread owns POOL_OUTS = 2 adjacent
// outputs of one row.  Output (yo, xo) is the mean of inputs (2 yo - py .. + 1, 2 xo - px .. + 1), py = H % 2, px = W % 2; index
// -1 is the zero padding, the far side never needs one.  Where the thread's four input columns all exist it fetches each row
// with load4; the sums are the same either way.
template <typename T>
__global__ void __launch_bounds__(MS_THREADS)
msssim_pool_kernel(const T* __restrict__ a, const T* __restrict__ b, long long in_plane, double* __restrict__ oa,
                   double* __restrict__ ob, long long out_plane, long long plane0, long long planes, int H, int W, int Ho, int Wo,
                   int groups_x) {
    const long long per_plane = (long long)Ho * groups_x;
    const long long idx = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (idx >= planes * per_plane) return;
    const long long plane = plane0 + idx / per_plane;
    const long long rem = idx % per_plane;
    const int yo = (int)(rem / groups_x), xo = (int)(rem % groups_x) * POOL_OUTS;       // xo < Wo
    const T* src = (blockIdx.y ? b : a) + plane * in_plane;
    double* dst = (blockIdx.y ? ob : oa) + plane * out_plane + (long long)yo * Wo + xo;
    const int y0 = 2 * yo - (H & 1), x0 = 2 * xo - (W & 1);
    const T* r1 = src + (long long)(y0 + 1) * W;    // row y0 + 1 <= H - 1
    const T* r0 = r1 - W;                           // dereferenced for y0 >= 0 only
    if (x0 >= 0 && x0 + 3 < W) {                    // both outputs exist (x0 + 3 <= W - 1) and neither touches the padding column
        double u[4] = {0.0, 0.0, 0.0, 0.0}, v[4];
        if (y0 >= 0) load4(r0 + x0, u);
        load4(r1 + x0, v);
        const double o0 = 0.25 * ((u[0] + u[1]) + (v[0] + v[1])), o1 = 0.25 * ((u[2] + u[3]) + (v[2] + v[3]));
        if (((unsigned long long)dst & 15) == 0) {
            *reinterpret_cast<double2*>(dst) = make_double2(o0, o1);
        } else {
            dst[0] = o0;
            dst[1] = o1;
        }
        return;
    }
    for (int j = 0; j < POOL_OUTS && xo + j < Wo; ++j) {
        const int x = x0 + 2 * j;                   // x + 1 <= W - 1
        const double x00 = (y0 >= 0 && x >= 0) ? (double)r0[x] : 0.0;
        const double x01 = y0 >= 0 ? (double)r0[x + 1] : 0.0;
        const double x10 = x >= 0 ? (double)r1[x] : 0.0;
        const double x11 = (double)r1[x + 1];
        dst[j] = 0.25 * ((x00 + x01) + (x10 + x11));
    }
}

// One 16x16 tile of one level's maps: the sums of the SSIM map and of the cs map over the tile's values inside the map.
template <typename T>
__device__ __forceinline__ void tile_sums(const T* __restrict__ pa, const T* __restrict__ pb, int H, int W, int y0, int x0,
                                          T* in_a, T* in_b, double (*rowf)[HALO * TILE], const double* tap, double c1, double c2,
                                          double& ssim_sum, double& cs_sum) {
    const int tid = threadIdx.x;
    for (int i = tid; i < HALO * HALO; i += MS_THREADS) {
        const int r = i / HALO, c = i % HALO;
        const int gy = y0 + r, gx = x0 + c;
        const bool inside = gy < H && gx < W;                 // beyond the plane: zeros, read by dropped lanes only
        const long long at = (long long)gy * W + gx;
        in_a[r * IN_LD + c] = inside ? pa[at] : (T)0;
        in_b[r * IN_LD + c] = inside ? pb[at] : (T)0;
    }
    __syncthreads();

    // along rows: HALO x TILE values of each quantity
    for (int i = tid; i < HALO * TILE; i += MS_THREADS) {
        const int r = i / TILE, c = i % TILE;
        const T* qa = in_a + r * IN_LD + c;
        const T* qb = in_b + r * IN_LD + c;
        double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const double t = tap[k], x1 = (double)qa[k], x2 = (double)qb[k];
            m1 = fma(t, x1, m1);
            m2 = fma(t, x2, m2);
            s11 = fma(t, x1 * x1, s11);          // level 0: exact products of widened floats; above: X * X rounded once, as the
            s22 = fma(t, x2 * x2, s22);          // definition filters it
            s12 = fma(t, x1 * x2, s12);
        }
        rowf[0][i] = m1; rowf[1][i] = m2; rowf[2][i] = s11; rowf[3][i] = s22; rowf[4][i] = s12;
    }
    __syncthreads();

    // along columns, the two maps
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
    const double cs = (2.0 * sigma12 + c2) / (sigma1_sq + sigma2_sq + c2);
    const double ssim = ((2.0 * mu1_mu2 + c1) / (mu1_sq + mu2_sq + c1)) * cs;
    const bool in_map = y0 + y < H - (WIN - 1) && x0 + x < W - (WIN - 1);
    ssim_sum = in_map ? ssim : 0.0;
    cs_sum = in_map ? cs : 0.0;
}

// partial[(plane * tiles + t) * 2 + {0, 1}] = the sums of the SSIM map and of the cs map over tile t of the plane, tiles =
// tile_end[levels-1].  One instantiation per input type, so that the fp32 level, three quarters of the work, keeps the LDS
// footprint (and with it the occupancy) of ssim_tile_kernel: <float> takes the tiles of level 0 (t_begin = 0, in_plane = H W),
// <double> those of every level above in one launch (t_begin = tile_end[0], in_plane = pyr_plane).
template <typename T>
__global__ void __launch_bounds__(MS_THREADS)
msssim_tile_kernel(const T* __restrict__ a, const T* __restrict__ b, long long in_plane, Pyramid P, int t_begin, int t_count,
                   long long plane0, const double* __restrict__ taps11, double c1, double c2, double* __restrict__ partial) {
    __shared__ T in_a[HALO * IN_LD];
    __shared__ T in_b[HALO * IN_LD];
    __shared__ double rowf[5][HALO * TILE];
    __shared__ double tap[WIN];
    __shared__ double wave_total[2][MS_WAVES];
    const int tiles = P.tile_end[P.levels - 1];
    const long long plane = plane0 + (long long)blockIdx.x / t_count;
    const int t = t_begin + (int)((long long)blockIdx.x % t_count);
    int level = 0;
    while (t >= P.tile_end[level]) ++level;                               // uniform over the workgroup; t < tile_end[levels - 1]
    const int tile = t - (level ? P.tile_end[level - 1] : 0);
    const int H = P.H[level], W = P.W[level], tiles_x = P.tiles_x[level];
    const int y0 = (tile / tiles_x) * TILE, x0 = (tile % tiles_x) * TILE;    // map (y, x) reads inputs (y .. y+10, x .. x+10)
    const long long base = plane * in_plane + P.pyr_off[level];          // pyr_off[0] = 0

    if (threadIdx.x < WIN) tap[threadIdx.x] = taps11[threadIdx.x];        // visible after the first barrier of tile_sums
    double ssim_sum, cs_sum;
    tile_sums<T>(a + base, b + base, H, W, y0, x0, in_a, in_b, rowf, tap, c1, c2, ssim_sum, cs_sum);
    block_sum2(ssim_sum, cs_sum, wave_total);
    if (threadIdx.x == 0) {
        double* p = partial + (plane * tiles + t) * 2;
        p[0] = ssim_sum;
        p[1] = cs_sum;
    }
}

// out[(plane * levels + level) * 2 + {0, 1}] = (sum of the level's tile totals) / (number of map values): lane t takes the
// level's tiles t, t + 256, ... in that order
__global__ void __launch_bounds__(MS_THREADS)
msssim_finish_kernel(const double* __restrict__ partial, Pyramid P, long long plane0, double* __restrict__ out) {
    __shared__ double wave_total[2][MS_WAVES];
    const long long plane = plane0 + blockIdx.x / P.levels;
    const int level = blockIdx.x % P.levels;
    const int tiles = P.tile_end[P.levels - 1];
    const int begin = level ? P.tile_end[level - 1] : 0, end = P.tile_end[level];
    const double* p = partial + plane * tiles * 2;
    double s = 0.0, c = 0.0;
    for (int i = begin + (int)threadIdx.x; i < end; i += MS_THREADS) {
        s += p[2 * i];
        c += p[2 * i + 1];
    }
    block_sum2(s, c, wave_total);
    if (threadIdx.x == 0) {
        const double count = (double)((long long)(P.H[level] - (WIN - 1)) * (P.W[level] - (WIN - 1)));
        double* o = out + (plane * P.levels + level) * 2;
        o[0] = s / count;
        o[1] = c / count;
    }
}

// EVC_OK and the filled table, or the code both exports return
__host__ int make_pyramid(int N, int H, int W, int levels, Pyramid* P) {
    if (N < 0 || levels < 1 || levels > MAX_LEVELS || H <= 0 || W <= 0) return EVC_EINVAL;
    if ((H < W ? H : W) <= (WIN - 1) * (1LL << (levels - 1))) return EVC_EINVAL;      // pytorch_msssim's assert; nothing is padded
    P->levels = levels;
    long long off = 0, tiles = 0;
    for (int l = 0; l < MAX_LEVELS; ++l) {
        if (l >= levels) {
            P->H[l] = P->W[l] = P->tiles_x[l] = 0;
            P->tile_end[l] = (int)tiles;
            P->pyr_off[l] = 0;
            continue;
        }
        P->H[l] = l ? (P->H[l - 1] + 1) / 2 : H;
        P->W[l] = l ? (P->W[l - 1] + 1) / 2 : W;
        const long long tx = (P->W[l] - (WIN - 1) + TILE - 1) / TILE, ty = (P->H[l] - (WIN - 1) + TILE - 1) / TILE;
        tiles += tx * ty;
        if (tiles > MAX_BLOCKS) return EVC_EUNSUPPORTED;
        P->tiles_x[l] = (int)tx;
        P->tile_end[l] = (int)tiles;
        P->pyr_off[l] = l ? off : 0;
        if (l) off += (long long)P->H[l] * P->W[l];
    }
    P->pyr_plane = off;
    return EVC_OK;
}

}  // namespace

extern "C" long long evc_msssim_workspace_bytes(int N, int H, int W, int levels) {
    Pyramid P;
    const int rc = make_pyramid(N, H, W, levels, &P);
    if (rc != EVC_OK) return rc;
    return (long long)N * (2 * P.pyr_plane + 2 * (long long)P.tile_end[levels - 1]) * (long long)sizeof(double);
}

extern "C" int evc_msssim_levels_f32(const float* a, const float* b, int N, int H, int W, int levels, const double* taps11,
                                     double c1, double c2, double* out, void* ws, void* stream) {
    Pyramid P;
    const int rc = make_pyramid(N, H, W, levels, &P);
    if (rc != EVC_OK) return rc;
    if (N == 0) return EVC_OK;
    if (!a || !b || !taps11 || !out || !ws) return EVC_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* pyr_a = (double*)ws;
    double* pyr_b = pyr_a + (long long)N * P.pyr_plane;
    double* partial = pyr_b + (long long)N * P.pyr_plane;
    const long long tiles = P.tile_end[levels - 1];

    for (int l = 0; l + 1 < levels; ++l) {
        const int Ho = P.H[l + 1], Wo = P.W[l + 1], groups_x = (Wo + POOL_OUTS - 1) / POOL_OUTS;
        const long long per_plane = (long long)Ho * groups_x;                         // threads per plane
        const long long per_launch = MAX_BLOCKS * MS_THREADS / per_plane;             // planes per launch; >= 1: level 0 has at
                                                                                      // most 2^30 tiles of 256, this one fewer threads
        for (long long p0 = 0; p0 < N; p0 += per_launch) {
            const long long n = N - p0 < per_launch ? N - p0 : per_launch;
            const dim3 grid((unsigned)((n * per_plane + MS_THREADS - 1) / MS_THREADS), 2);
            double* oa = pyr_a + P.pyr_off[l + 1];
            double* ob = pyr_b + P.pyr_off[l + 1];
            if (l == 0)
                hipLaunchKernelGGL(msssim_pool_kernel<float>, grid, dim3(MS_THREADS), 0, s, a, b, (long long)H * W, oa, ob,
                                   P.pyr_plane, p0, n, H, W, Ho, Wo, groups_x);
            else
                hipLaunchKernelGGL(msssim_pool_kernel<double>, grid, dim3(MS_THREADS), 0, s, (const double*)pyr_a + P.pyr_off[l],
                                   (const double*)pyr_b + P.pyr_off[l], P.pyr_plane, oa, ob, P.pyr_plane, p0, n, P.H[l], P.W[l], Ho,
                                   Wo, groups_x);
        }
    }
    const long long per_launch = MAX_BLOCKS / tiles;          // planes per launch: a plane's numbers do not depend on it
    for (long long p0 = 0; p0 < N; p0 += per_launch) {
        const long long n = N - p0 < per_launch ? N - p0 : per_launch;
        const int t0 = P.tile_end[0], t1 = (int)tiles - t0;                // tiles of level 0, of the levels above
        hipLaunchKernelGGL(msssim_tile_kernel<float>, dim3((unsigned)(n * t0)), dim3(MS_THREADS), 0, s, a, b, (long long)H * W, P, 0,
                           t0, p0, taps11, c1, c2, partial);
        if (t1 > 0)
            hipLaunchKernelGGL(msssim_tile_kernel<double>, dim3((unsigned)(n * t1)), dim3(MS_THREADS), 0, s, (const double*)pyr_a,
                               (const double*)pyr_b, P.pyr_plane, P, t0, t1, p0, taps11, c1, c2, partial);
        hipLaunchKernelGGL(msssim_finish_kernel, dim3((unsigned)(n * levels)), dim3(MS_THREADS), 0, s, (const double*)partial, P,
                           p0, out);
    }
    return EVC_LAUNCH_OK();
}
