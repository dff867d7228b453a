// tile.hip -- whole frames through a fixed-size model: cut a frame into overlapping S x S tiles, blend decoded tiles back,
// DESIGN.md section 8c "Whole frames".
//
//   evc_tile_gather_u8   src (N, 3, H, W) uint8 -> dst (ny * nx, N, 3, S, S) uint8, a copy:
//                        dst[t][n][c][y][x] = src[n][c][min(oy[ty] + y, H - 1)][min(ox[tx] + x, W - 1)],  t = ty * nx + tx
//   evc_tile_blend_f32   tiles (ny * nx, N, 3, S, S) fp32 -> out (N, 3, H, W) fp32, the tent-weighted mean of the tiles that
//                        cover a pixel
//   evc_tile_gather_f32  the gather for fp32 planes of any channel count: src (N, C, H, W) -> dst (ny * nx, N, C, S, S), the same
//                        copy (joint generation, tiled.py: the noisy state and the conditioning frames of a whole canvas)
//
// The blend of one output pixel (y, x): with the integer tent t(i) = min(i + 1, S - i), the tiles that cover the pixel are
// visited in ascending tile index; acc = acc + float(t(ly) * t(lx)) * v (the product rounded, then the sum: no contraction),
// den = the integer sum of the weights, out = acc / float(den), IEEE division.  A tile that does not cover the pixel is not
// read, so the padding samples of an axis shorter than S never enter, and a NaN / inf reaches the pixels of its own tile only.
// No atomics: a thread owns 4 adjacent output pixels (one 16-byte store; W % 4 == 0) or one, and an output depends on its own
// frame's tiles and the grid only.
//
// Both kernels move bytes.  The gather gives a thread 16 adjacent destination bytes (S % 16 == 0; one byte otherwise): they
// move as one 16-byte load and one 16-byte store where all 16 source bytes lie in the row and the source address is 16-byte
// aligned, byte by byte under the clamp elsewhere -- an odd W or an origin that is no multiple of 16 takes the same kernel.
// The blend reads a tile's 4 values as one 16-byte load where the group lies inside the tile at an aligned address, else the
// covered ones one by one.  The origins are read from the device arrays and held inside [0, max(L - S, 0)] whatever they
// say, so nothing outside src / tiles is read even if they differ from the host arrays that were checked.
// The fp32 gather is ONE kernel for every shape: a thread owns 4 consecutive floats of the packed destination.  Where the four
// lie in one tile row, their source columns lie inside the row and both addresses are 16-byte aligned they move as one
// 16-byte load and store; elsewhere (odd W, an origin or an S that is no multiple of 4, the edge replication of a short axis,
// a group that runs over the end of a tile row) each float is located on its own and moves alone under the clamp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/evc_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int SIDE = 1 << 24;
constexpr int ORIGINS_LDS = 1024;             // column origins a blend workgroup holds in LDS

__device__ __forceinline__ int origin(const int* __restrict__ o, int k, int L, int S) {
    return min(max(o[k], 0), max(L - S, 0));
}

// The first tile of an axis whose samples [o, o + S) reach sample p, i.e. the smallest k with o[k] + S > p (n - 1 when none
// does).  The origins increase, so the tiles that cover p are k, k + 1, ... while o <= p.  The walk starts where evenly spaced
// origins would put the answer -- a guess that only shortens the walk, a few loads instead of n; the result does not depend
// on it.
__device__ __forceinline__ int first_reaching(const int* __restrict__ o, int n, int L, int S, int p) {
    int k = 0;
    if (p >= S && n > 1) k = min((int)__fdividef((float)(p - S + 1) * (float)(n - 1), (float)max(L - S, 1)), n - 1);
    while (k > 0 && origin(o, k - 1, L, S) + S > p) --k;
    while (k < n - 1 && origin(o, k, L, S) + S <= p) ++k;
    return k;
}

// V = 16: S % 16 == 0 and dst 16-byte aligned; V = 1: anything.  One thread per V destination bytes.
template <int V>
__global__ void __launch_bounds__(THREADS)
tile_gather_kernel(const uint8_t* __restrict__ src, int N, int H, int W, int S, int nx, const int* __restrict__ oy,
                   const int* __restrict__ ox, uint8_t* __restrict__ dst, long long total) {
    const long long idx = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const int sg = S / V;
    const int x = (int)(idx % sg) * V;
    long long r = idx / sg;
    const int y = (int)(r % S);
    r /= S;
    const int plane = (int)(r % (3LL * N));
    const int t = (int)(r / (3LL * N));
    const int y0 = origin(oy, t / nx, H, S), x0 = origin(ox, t % nx, W, S);
    const uint8_t* row = src + ((long long)plane * H + min(y0 + y, H - 1)) * W;
    uint8_t* d = dst + idx * V;
    if constexpr (V == 16) {
        const uint8_t* s = row + x0 + x;
        if (x0 + x + 16 <= W && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
            *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
        } else {
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w[j] = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) w[j] |= (uint32_t)row[min(x0 + x + 4 * j + b, W - 1)] << (8 * b);
            }
            *reinterpret_cast<uint4*>(d) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        *d = row[min(x0 + x, W - 1)];
    }
}

// Where float ``idx`` of the packed destination (t, plane, y, x) comes from: its source row (clamped) and, in x0 / x, the tile's
// column origin and the column inside the tile.  planes = N * C.
__device__ __forceinline__ const uint32_t* gather_row(const uint32_t* __restrict__ src, long long idx, long long planes, int H, int W,
                                                      int S, int nx, const int* __restrict__ oy, const int* __restrict__ ox, int& x0,
                                                      int& x) {
    x = (int)(idx % S);
    long long r = idx / S;
    const int y = (int)(r % S);
    r /= S;
    const long long plane = r % planes, t = r / planes;
    const int y0 = origin(oy, (int)(t / nx), H, S);
    x0 = origin(ox, (int)(t % nx), W, S);
    return src + (plane * H + min(y0 + y, H - 1)) * W;
}

// One thread per 4 consecutive destination floats (the last group of an odd total is short).  The samples move as 32-bit words:
// a copy, whatever their bits mean.
__global__ void __launch_bounds__(THREADS)
tile_gather_f32_kernel(const uint32_t* __restrict__ src, long long planes, int H, int W, int S, int nx, const int* __restrict__ oy,
                       const int* __restrict__ ox, uint32_t* __restrict__ dst, long long total) {
    const long long g = ((long long)blockIdx.x * THREADS + threadIdx.x) * 4;
    if (g >= total) return;
    int x0, x;
    const uint32_t* row = gather_row(src, g, planes, H, W, S, nx, oy, ox, x0, x);
    const uint32_t* s = row + x0 + x;
    uint32_t* d = dst + g;
    if (x + 4 <= S && x0 + x + 4 <= W && ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) {
        *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
        return;
    }
    for (int j = 0; j < 4 && g + j < total; ++j) {
        row = gather_row(src, g + j, planes, H, W, S, nx, oy, ox, x0, x);
        d[j] = row[min(x0 + x, W - 1)];
    }
}

// V = 4: W % 4 == 0 and out 16-byte aligned; V = 1: anything.  One thread per V adjacent output pixels, one workgroup per
// stretch of one output row (grid: rows * xblocks, rows = 3 N H), so the row, its plane and the rows of tiles that cover it are
// the same for the whole workgroup: scalar work.  The column origins are walked per thread; up to ORIGINS_LDS of them are
// staged in LDS first (any more are read where they lie).
template <int V>
__global__ void __launch_bounds__(THREADS)
tile_blend_kernel(const float* __restrict__ tiles, int N, int H, int W, int S, int ny, int nx, const int* __restrict__ oy,
                  const int* __restrict__ ox_global, float* __restrict__ out, int xblocks) {
    __shared__ int ox_lds[ORIGINS_LDS];
    const int* ox = ox_global;
    if (nx <= ORIGINS_LDS) {
        for (int i = threadIdx.x; i < nx; i += blockDim.x) ox_lds[i] = ox_global[i];
        __syncthreads();
        ox = ox_lds;
    }
    const int x = (int)((blockIdx.x % xblocks) * blockDim.x + threadIdx.x) * V;
    if (x >= W) return;
    const long long row = blockIdx.x / xblocks;          // (n * 3 + c) * H + y
    const int y = (int)(row % H);
    const long long plane = row / H;
    const long long tile_stride = 3LL * N * S * S;       // floats between two tiles
    float acc[V];
    long long den[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { acc[j] = 0.0f; den[j] = 0; }
    const int tx0 = first_reaching(ox, nx, W, S, x);     // of the group's first pixel: no earlier tile reaches any of the group
    for (int ty = first_reaching(oy, ny, H, S, y); ty < ny; ++ty) {
        const int ly = y - origin(oy, ty, H, S);
        if (ly < 0) break;                               // origins increase: no later row of tiles covers y
        if (ly >= S) continue;
        const int wy = min(ly + 1, S - ly);
        const float* trow = tiles + ((long long)ty * nx * tile_stride + (plane * S + ly) * S);
        for (int tx = tx0; tx < nx; ++tx) {
            const int lx = x - origin(ox, tx, W, S);     // of the group's first pixel
            if (lx + V - 1 < 0) break;
            if (lx >= S) continue;
            const float* p = trow + tx * tile_stride + lx;
            float v[V];
            bool in[V], whole = false;
            if constexpr (V == 4) {
                whole = lx >= 0 && lx + 4 <= S && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
                if (whole) {
                    const float4 q = *reinterpret_cast<const float4*>(p);
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                    in[0] = in[1] = in[2] = in[3] = true;
                }
            }
            if (!whole) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    in[j] = lx + j >= 0 && lx + j < S;
                    v[j] = in[j] ? p[j] : 0.0f;
                }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (in[j]) {
                    // both factors are below 2^24, so the float product is the integer product rounded once: float(t(ly) t(lx))
                    const int wx = min(lx + j + 1, S - lx - j);
                    acc[j] = acc[j] + ((float)wy * (float)wx) * v[j];
                    den[j] += (long long)wy * wx;
                }
            }
        }
    }
    float* o = out + (row * W + x);
    if constexpr (V == 4)
        *reinterpret_cast<float4*>(o) = make_float4(acc[0] / (float)den[0], acc[1] / (float)den[1], acc[2] / (float)den[2],
                                                    acc[3] / (float)den[3]);
    else
        *o = acc[0] / (float)den[0];
}

// One axis: n origins inside [0, max(L - S, 0)], strictly increasing.  cover: also the first at 0, steps of at most S and the
// last at max(L - S, 0), so that every sample of the axis lies in a tile (the blend divides by the weight it found).
bool bad_axis(const int* o, int n, int L, int S, bool cover) {
    const int last = L > S ? L - S : 0;
    for (int k = 0; k < n; ++k) {
        if (o[k] < 0 || o[k] > last) return true;
        if (k && (o[k] <= o[k - 1] || (cover && o[k] - o[k - 1] > S))) return true;
    }
    return cover && (o[0] != 0 || o[n - 1] != last);
}

bool bad_grid(int N, int H, int W, int S, int ny, int nx, const int* oy, const int* ox, bool cover) {
    return !oy || !ox || N <= 0 || H <= 0 || W <= 0 || S <= 0 || ny <= 0 || nx <= 0 || N > SIDE || H > SIDE || W > SIDE ||
           S > SIDE || ny > SIDE || nx > SIDE || 3LL * N * H > (1LL << 62) / W || bad_axis(oy, ny, H, S, cover) || bad_axis(ox, nx, W, S, cover);
}

bool blocks_of(long long total, unsigned& blocks) {
    const long long b = (total + THREADS - 1) / THREADS;
    blocks = (unsigned)b;
    return b <= 0x7FFFFFFFLL;
}

// ny * nx * N * 3 * S * S elements, or -1 when that leaves 2^62
long long tile_elements(int N, int S, int ny, int nx) {
    const long long tiles = (long long)ny * nx, per = 3LL * N * S;       // each below 2^48 and 2^50
    if (tiles > (1LL << 62) / per / S) return -1;
    return tiles * per * S;
}

}  // namespace

extern "C" int evc_tile_grid_check(int N, int H, int W, int S, int ny, int nx, const int* oy_host, const int* ox_host, int cover) {
    if (bad_grid(N, H, W, S, ny, nx, oy_host, ox_host, cover != 0) || tile_elements(N, S, ny, nx) < 0) return EVC_EINVAL;
    return EVC_OK;
}

extern "C" int evc_tile_gather_u8(const unsigned char* src, int N, int H, int W, int S, int ny, int nx, const int* oy_host,
                                  const int* ox_host, const int* oy, const int* ox, unsigned char* dst, void* stream) {
    if (!src || !dst || !oy || !ox || bad_grid(N, H, W, S, ny, nx, oy_host, ox_host, false)) return EVC_EINVAL;
    const long long bytes = tile_elements(N, S, ny, nx);
    if (bytes < 0) return EVC_EINVAL;
    const bool vec = S % 16 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const long long total = bytes / (vec ? 16 : 1);
    unsigned blocks;
    if (!blocks_of(total, blocks)) return EVC_EINVAL;
    if (vec)
        hipLaunchKernelGGL(tile_gather_kernel<16>, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, src, N, H, W, S, nx, oy, ox,
                           dst, total);
    else
        hipLaunchKernelGGL(tile_gather_kernel<1>, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, src, N, H, W, S, nx, oy, ox,
                           dst, total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_tile_gather_f32(const float* src, int N, int C, int H, int W, int S, int ny, int nx, const int* oy_host,
                                   const int* ox_host, const int* oy, const int* ox, float* dst, void* stream) {
    if (!src || !dst || !oy || !ox || C <= 0 || C > SIDE || bad_grid(N, H, W, S, ny, nx, oy_host, ox_host, false)) return EVC_EINVAL;
    const long long planes = (long long)N * C;                                  // below 2^48
    if (planes > (1LL << 62) / H / W || planes > (1LL << 62) / S / S) return EVC_EINVAL;       // src and one tile's floats below 2^62
    const long long per_tile = planes * S * S, tiles = (long long)ny * nx;
    if (tiles > (1LL << 62) / per_tile) return EVC_EINVAL;
    const long long total = tiles * per_tile;
    unsigned blocks;
    if (!blocks_of((total + 3) / 4, blocks)) return EVC_EINVAL;
    hipLaunchKernelGGL(tile_gather_f32_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(src), planes, H, W, S, nx, oy, ox, reinterpret_cast<uint32_t*>(dst), total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_tile_blend_f32(const float* tiles, int N, int H, int W, int S, int ny, int nx, const int* oy_host,
                                  const int* ox_host, const int* oy, const int* ox, float* out, void* stream) {
    if (!tiles || !out || !oy || !ox || bad_grid(N, H, W, S, ny, nx, oy_host, ox_host, true)) return EVC_EINVAL;
    if (tile_elements(N, S, ny, nx) < 0) return EVC_EINVAL;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const int groups = W / (vec ? 4 : 1);                                    // threads a row needs
    const int threads = groups >= THREADS ? THREADS : (groups + 63) / 64 * 64;
    const int xblocks = (groups + threads - 1) / threads;
    const long long blocks = 3LL * N * H * xblocks;
    if (blocks > 0x7FFFFFFFLL) return EVC_EINVAL;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), 0, (hipStream_t)stream, tiles, N, H, W, S, ny, nx, oy, ox,
                           out, xblocks);
    };
    vec ? launch(tile_blend_kernel<4>) : launch(tile_blend_kernel<1>);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}
