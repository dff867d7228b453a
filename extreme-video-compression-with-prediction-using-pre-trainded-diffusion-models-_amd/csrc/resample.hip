// resample.hip -- Pillow's 8-bit resize (ImagingResample, 8 bits per channel) as two integer passes, DESIGN.md section 8c.
//
//   evc_resample_h_u8   filters along the contiguous axis: (planes, rows, cols) -> (planes, rows, n_out)
//   evc_resample_v_u8   filters along the row axis:        (planes, rows, cols) -> (planes, n_out, cols)
//
// Output index i of either pass is clamp((2^21 + sum_{x < n} src[xmin + x] * k[i][x]) >> 22, 0, 255) with (xmin, n) =
// bounds[i] and k[i] = coeffs + i * ksize, all in int32 (the caller's tables guarantee the sum fits: lib.resample_tables).
// The shift is arithmetic, so a negative sum goes to 0.  There is no float and no atomic anywhere: an output byte is a function
// of its own row (column) of its own plane and of the tables, whatever else the launch holds.
//
// Both passes move bytes.  The source is a window into a larger image (plane and row strides in bytes, no alignment asked),
// so the horizontal pass stages whole source rows in LDS: the row is cut into the 16-byte chunks of its ALIGNED addresses, a
// chunk that lies inside the row moves as one 16-byte load and one 16-byte LDS store, the chunk at the head and the one at the
// tail byte by byte under a bounds check -- nothing outside [row, row + cols) is read.  In LDS the row keeps its misalignment
// (column c at a + c, a = address & 15).  A thread then owns one output column for RPT rows, so a coefficient is read once for
// RPT products; the table sits in LDS with an odd row stride (consecutive columns on different banks) when it fits beside the
// rows, else it is read through L2.  Rows too long for LDS take the direct kernel, one thread per output, everything through
// the cache.  The vertical pass gives a thread 4 adjacent columns (one dword per source row, where the pointers allow it, else
// one column) and walks down; consecutive lanes read consecutive bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/evc_hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int RPT = 4;                        // rows per thread, horizontal pass
constexpr int LDS_BYTES = 64 * 1024;          // rows + table of one workgroup
constexpr int PRECISION = 22, HALF = 1 << (PRECISION - 1);

__device__ __forceinline__ unsigned clip8(int acc) {
    const int v = acc >> PRECISION;
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// (xmin, n) of output i, held inside [0, len) and ksize whatever the table says.
__device__ __forceinline__ void window(const int* __restrict__ bounds, int i, int len, int ksize, int& xmin, int& n) {
    xmin = min(max(bounds[2 * i], 0), len);
    n = max(min(min(bounds[2 * i + 1], ksize), len - xmin), 0);
}

// grid: planes * row_blocks workgroups; dynamic LDS: block_rows * lrow bytes of rows, then (TABLE_LDS) n_out * kst ints.
template <bool TABLE_LDS>
__global__ void __launch_bounds__(THREADS)
resample_h_kernel(const uint8_t* __restrict__ src, int rows, int cols, long long plane_stride, long long row_stride,
                  const int* __restrict__ bounds, const int* __restrict__ coeffs, int ksize, int n_out, uint8_t* __restrict__ dst,
                  int row_blocks, int block_rows, int lrow, int kst) {
    extern __shared__ __align__(16) uint8_t smem[];
    uint8_t* tile = smem;
    int* table = reinterpret_cast<int*>(smem + (size_t)block_rows * lrow);
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / row_blocks, r0 = (blockIdx.x % row_blocks) * block_rows;
    const int nr = min(block_rows, rows - r0);
    const uint8_t* base = src + (long long)plane * plane_stride + (long long)r0 * row_stride;
    const int chunks = lrow / 16;
    for (int i = tid; i < nr * chunks; i += THREADS) {
        const int r = i / chunks, c = i % chunks;
        const uint8_t* row = base + (long long)r * row_stride;
        const int g0 = 16 * c - (int)(reinterpret_cast<uintptr_t>(row) & 15);      // the chunk's first byte as a column of the row
        uint8_t* l = tile + (size_t)r * lrow + 16 * c;
        if (g0 >= 0 && g0 + 16 <= cols) {
            *reinterpret_cast<uint4*>(l) = *reinterpret_cast<const uint4*>(row + g0);
        } else {
            for (int b = 0; b < 16; ++b)
                if (g0 + b >= 0 && g0 + b < cols) l[b] = row[g0 + b];
        }
    }
    if (TABLE_LDS)
        for (int i = tid; i < n_out * ksize; i += THREADS) table[(i / ksize) * kst + i % ksize] = coeffs[i];
    __syncthreads();
    const int groups = block_rows / RPT;
    for (int item = tid; item < n_out * groups; item += THREADS) {
        const int xx = item % n_out, rg = item / n_out;
        int xmin, n;
        window(bounds, xx, cols, ksize, xmin, n);
        const int* k = TABLE_LDS ? table + xx * kst : coeffs + (long long)xx * ksize;
        const uint8_t* p[RPT];
        int acc[RPT];
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            const int r = rg * RPT + j;       // rows past nr hold stale LDS: filtered, never stored
            p[j] = tile + (size_t)r * lrow + (reinterpret_cast<uintptr_t>(base + (long long)r * row_stride) & 15) + xmin;
            acc[j] = HALF;
        }
        for (int x = 0; x < n; ++x) {
            const int kv = k[x];
#pragma unroll
            for (int j = 0; j < RPT; ++j) acc[j] += (int)p[j][x] * kv;
        }
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            const int r = rg * RPT + j;
            if (r < nr) dst[((size_t)plane * rows + r0 + r) * n_out + xx] = (uint8_t)clip8(acc[j]);
        }
    }
}

// One thread per output, source and table through the cache: rows that LDS cannot hold.
__global__ void __launch_bounds__(THREADS)
resample_h_direct_kernel(const uint8_t* __restrict__ src, int rows, int cols, long long plane_stride, long long row_stride,
                         const int* __restrict__ bounds, const int* __restrict__ coeffs, int ksize, int n_out,
                         uint8_t* __restrict__ dst, long long total) {
    const long long idx = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const int xx = (int)(idx % n_out);
    const long long pr = idx / n_out;
    const int r = (int)(pr % rows), plane = (int)(pr / rows);
    int xmin, n;
    window(bounds, xx, cols, ksize, xmin, n);
    const uint8_t* p = src + (long long)plane * plane_stride + (long long)r * row_stride + xmin;
    const int* k = coeffs + (long long)xx * ksize;
    int acc = HALF;
    for (int x = 0; x < n; ++x) acc += (int)p[x] * k[x];
    dst[idx] = (uint8_t)clip8(acc);
}

// V = 4: cols % 4 == 0 and src, both strides and dst 4-byte aligned (uniform over the launch); V = 1: anything.
template <int V>
__global__ void __launch_bounds__(THREADS)
resample_v_kernel(const uint8_t* __restrict__ src, int rows, int cols, long long plane_stride, long long row_stride,
                  const int* __restrict__ bounds, const int* __restrict__ coeffs, int ksize, int n_out, uint8_t* __restrict__ dst,
                  long long total) {
    const long long idx = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const int cg = cols / V;
    const int c = (int)(idx % cg) * V;
    const long long py = idx / cg;
    const int yy = (int)(py % n_out), plane = (int)(py / n_out);
    int ymin, n;
    window(bounds, yy, rows, ksize, ymin, n);
    const uint8_t* p = src + (long long)plane * plane_stride + (long long)ymin * row_stride + c;
    const int* k = coeffs + (long long)yy * ksize;
    int acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = HALF;
    for (int x = 0; x < n; ++x) {
        const int kv = k[x];
        if constexpr (V == 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(p + (long long)x * row_stride);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += (int)((w >> (8 * j)) & 255u) * kv;
        } else {
            acc[0] += (int)p[(long long)x * row_stride] * kv;
        }
    }
    uint8_t* o = dst + ((size_t)plane * n_out + yy) * cols + c;
    if constexpr (V == 4)
        *reinterpret_cast<uint32_t*>(o) = clip8(acc[0]) | (clip8(acc[1]) << 8) | (clip8(acc[2]) << 16) | (clip8(acc[3]) << 24);
    else
        *o = (uint8_t)clip8(acc[0]);
}

bool bad_shape(const void* src, int planes, int rows, int cols, long long plane_stride, long long row_stride, const int* bounds,
               const int* coeffs, int ksize, int n_out, const void* dst) {
    constexpr int SIDE = 1 << 24;
    return !src || !dst || !bounds || !coeffs || planes <= 0 || rows <= 0 || cols <= 0 || ksize <= 0 || n_out <= 0 ||
           rows > SIDE || cols > SIDE || n_out > SIDE || row_stride < cols || plane_stride < 0 || (planes > 1 && plane_stride < (long long)(rows - 1) * row_stride + cols) ||
           (long long)n_out * ksize > 0x7FFFFFFFLL;
}

bool blocks_of(long long total, unsigned& blocks) {
    const long long b = (total + THREADS - 1) / THREADS;
    blocks = (unsigned)b;
    return b <= 0x7FFFFFFFLL;
}

}  // namespace

extern "C" int evc_resample_h_u8(const unsigned char* src, int planes, int rows, int cols, long long plane_stride,
                                 long long row_stride, const int* bounds, const int* coeffs, int ksize, int n_out,
                                 unsigned char* dst, void* stream) {
    if (bad_shape(src, planes, rows, cols, plane_stride, row_stride, bounds, coeffs, ksize, n_out, dst)) return EVC_EINVAL;
    const long long lrow = ((long long)cols + 30) / 16 * 16;         // every aligned 16-byte chunk the row touches, at any address
    if (RPT * lrow <= LDS_BYTES) {
        const int kst = ksize | 1;
        const long long table = (long long)n_out * kst * 4;
        const bool table_lds = RPT * lrow + table <= LDS_BYTES;
        const long long room = LDS_BYTES - (table_lds ? table : 0);
        // enough rows that the n_out * rows / RPT items fill the workgroup, as far as LDS and the image go
        long long block_rows = ((4LL * THREADS + n_out - 1) / n_out + RPT - 1) / RPT * RPT;
        block_rows = block_rows < 2 * RPT ? 2 * RPT : (block_rows > 64 ? 64 : block_rows);
        while (block_rows > RPT && (block_rows * lrow > room || block_rows - RPT >= rows)) block_rows -= RPT;
        const long long row_blocks = (rows + block_rows - 1) / block_rows;
        if (row_blocks * planes > 0x7FFFFFFFLL) return EVC_EINVAL;
        const dim3 grid((unsigned)(row_blocks * planes));
        const size_t lds = (size_t)(block_rows * lrow + (table_lds ? table : 0));
        if (table_lds)
            hipLaunchKernelGGL(resample_h_kernel<true>, grid, dim3(THREADS), lds, (hipStream_t)stream, src, rows, cols, plane_stride,
                               row_stride, bounds, coeffs, ksize, n_out, dst, (int)row_blocks, (int)block_rows, (int)lrow, kst);
        else
            hipLaunchKernelGGL(resample_h_kernel<false>, grid, dim3(THREADS), lds, (hipStream_t)stream, src, rows, cols, plane_stride,
                               row_stride, bounds, coeffs, ksize, n_out, dst, (int)row_blocks, (int)block_rows, (int)lrow, kst);
    } else {
        const long long total = (long long)planes * rows * n_out;
        unsigned blocks;
        if (!blocks_of(total, blocks)) return EVC_EINVAL;
        hipLaunchKernelGGL(resample_h_direct_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, src, rows, cols, plane_stride,
                           row_stride, bounds, coeffs, ksize, n_out, dst, total);
    }
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}

extern "C" int evc_resample_v_u8(const unsigned char* src, int planes, int rows, int cols, long long plane_stride,
                                 long long row_stride, const int* bounds, const int* coeffs, int ksize, int n_out,
                                 unsigned char* dst, void* stream) {
    if (bad_shape(src, planes, rows, cols, plane_stride, row_stride, bounds, coeffs, ksize, n_out, dst)) return EVC_EINVAL;
    const bool vec = cols % 4 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) |
                                        (uintptr_t)plane_stride | (uintptr_t)row_stride) & 3) == 0;
    const long long total = (long long)planes * n_out * (cols / (vec ? 4 : 1));
    unsigned blocks;
    if (!blocks_of(total, blocks)) return EVC_EINVAL;
    if (vec)
        hipLaunchKernelGGL(resample_v_kernel<4>, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, src, rows, cols, plane_stride,
                           row_stride, bounds, coeffs, ksize, n_out, dst, total);
    else
        hipLaunchKernelGGL(resample_v_kernel<1>, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, src, rows, cols, plane_stride,
                           row_stride, bounds, coeffs, ksize, n_out, dst, total);
    return hipGetLastError() == hipSuccess ? EVC_OK : EVC_ELAUNCH;
}
