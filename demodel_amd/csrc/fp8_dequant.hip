// CDNA4 FP8 block-scaled dequant (safetensors F8_E4M3 -> bf16 / f32).
//
// FP8 checkpoints ship a 2-D weight of OCP e4m3fn bytes plus a scale tensor
// (one scale per block_rows x block_cols block; per-tensor and per-row are
// the degenerate blocks).  The landed blob already sits in HBM, so widening
// is one pass: 1 B in, 2 B (bf16) or 4 B (f32) out, one f32 multiply and one
// round-to-nearest-even per element.
//
// Work unit: a "run" of up to 16 contiguous elements of one row, one run per
// lane.  A 64x4 workgroup covers 64 consecutive runs (one wave, 1 KiB of
// codes) of 4 rows; the grid strides over rows in y and over a row's runs in
// x, so no lane ever divides a flat index back into (row, column).  The
// block a run falls in is a shift when the block size is a power of two or
// covers the whole dimension (every checkpoint seen), a division otherwise.
//
// Safetensors places 1-byte tensors at any byte offset and cols may be odd,
// so neither side is assumed aligned: a full run takes the widest load/store
// its address allows and drops to narrower ones otherwise; a ragged row tail
// goes element by element.  The scale is read once per run when
// block_cols >= 16 (a run then spans at most two block columns), with byte
// loads unless its address happens to be aligned.

#include <hip/hip_runtime.h>

namespace {

constexpr int kRun = 16;           // elements per lane per iteration
constexpr int kLanesX = 64;        // runs of one row per workgroup
constexpr int kRowsPerBlock = 4;   // rows per workgroup
constexpr int kMaxGridX = 64;      // x covers 64*64*16 = 65536 cols a pass
constexpr int kMaxBlocks = 8192;   // measured best of 1k..64k; stride beyond

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
  uint32_t x = __float_as_uint(f);
  if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x40);
  uint32_t lsb = (x >> 16) & 1u;
  return (uint16_t)((x + 0x7fffu + lsb) >> 16);
}

// 64-bit division is a long VALU sequence; every real tensor fits 32 bits
__device__ __forceinline__ uint64_t udiv(uint64_t a, uint64_t b) {
  if (((a | b) >> 32) == 0) return (uint32_t)a / (uint32_t)b;
  return a / b;
}

// index / block: shift >= 0 replaces the division (see block_shift)
__device__ __forceinline__ uint64_t block_of(uint64_t i, uint64_t block,
                                             int shift) {
  return shift >= 0 ? i >> shift : udiv(i, block);
}

// scale element idx as f32; byte loads unless the address is aligned
__device__ __forceinline__ float load_scale(const uint8_t* scale,
                                            uint64_t idx, int dtype) {
  if (dtype == 0) {
    const uint8_t* p = scale + idx * 4;
    if ((((uint64_t)p) & 3) == 0) return *(const float*)p;
    uint32_t b = (uint32_t)p[0] | ((uint32_t)p[1] << 8) |
                 ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    return __uint_as_float(b);
  }
  const uint8_t* p = scale + idx * 2;
  uint16_t b = (uint16_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8));
  if (dtype == 1) return __uint_as_float((uint32_t)b << 16);
  return (float)__builtin_bit_cast(_Float16, b);
}

template <bool DST_F32>
__global__ void __launch_bounds__(kLanesX * kRowsPerBlock)
fp8_block_dequant_kernel(const uint8_t* __restrict__ src,
                         const uint8_t* __restrict__ scale, int scale_dtype,
                         void* __restrict__ dst, uint64_t rows, uint64_t cols,
                         uint64_t block_rows, uint64_t block_cols,
                         int row_shift, int col_shift, uint64_t scale_cols,
                         uint64_t runs_per_row) {
  for (uint64_t r = (uint64_t)blockIdx.y * kRowsPerBlock + threadIdx.y;
       r < rows; r += (uint64_t)gridDim.y * kRowsPerBlock) {
    const uint64_t srow = block_of(r, block_rows, row_shift) * scale_cols;
    for (uint64_t k = (uint64_t)blockIdx.x * kLanesX + threadIdx.x;
         k < runs_per_row; k += (uint64_t)gridDim.x * kLanesX) {
      const uint64_t c0 = k * kRun;
      const uint64_t left = cols - c0;
      const int n = left < (uint64_t)kRun ? (int)left : kRun;
      const uint64_t e0 = r * cols + c0;  // first element of the run

      // ---- load up to 16 code bytes into four words
      const uint8_t* s = src + e0;
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (n == kRun && (((uint64_t)s) & 15) == 0) {
        uint4 v = *(const uint4*)s;
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
      } else if (n == kRun && (((uint64_t)s) & 3) == 0) {
        const uint32_t* s1 = (const uint32_t*)s;
        w[0] = s1[0]; w[1] = s1[1]; w[2] = s1[2]; w[3] = s1[3];
      } else {
#pragma unroll
        for (int j = 0; j < kRun; ++j)
          if (j < n) w[j >> 2] |= (uint32_t)s[j] << ((j & 3) * 8);
      }

      // ---- decode (gfx950 v_cvt_pk_f32_fp8 is OCP e4m3fn)
      float f[kRun];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[q], false);
        auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[q], true);
        f[q * 4 + 0] = lo[0]; f[q * 4 + 1] = lo[1];
        f[q * 4 + 2] = hi[0]; f[q * 4 + 3] = hi[1];
      }

      // ---- scale: exactly one f32 multiply per element
      if (block_cols >= (uint64_t)kRun) {
        const uint64_t bc0 = block_of(c0, block_cols, col_shift);
        // elements of this run that lie before the next block column
        const uint64_t before = (bc0 + 1) * block_cols - c0;
        const float s0 = load_scale(scale, srow + bc0, scale_dtype);
        if (before >= (uint64_t)n) {
#pragma unroll
          for (int j = 0; j < kRun; ++j) f[j] *= s0;
        } else {
          const float s1 = load_scale(scale, srow + bc0 + 1, scale_dtype);
#pragma unroll
          for (int j = 0; j < kRun; ++j)
            f[j] *= ((uint64_t)j < before) ? s0 : s1;
        }
      } else {
        // narrow blocks (never seen in checkpoints): a lookup per element
#pragma unroll
        for (int j = 0; j < kRun; ++j)
          if (j < n)
            f[j] *= load_scale(
                scale, srow + block_of(c0 + j, block_cols, col_shift),
                scale_dtype);
      }

      // ---- store
      if (DST_F32) {
        float* d = (float*)dst + e0;
        if (n == kRun && (((uint64_t)d) & 15) == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            ((float4*)d)[q] = make_float4(f[q * 4], f[q * 4 + 1],
                                          f[q * 4 + 2], f[q * 4 + 3]);
        } else {
#pragma unroll
          for (int j = 0; j < kRun; ++j)
            if (j < n) d[j] = f[j];
        }
      } else {
        uint16_t* d = (uint16_t*)dst + e0;
        uint16_t o[kRun];
#pragma unroll
        for (int j = 0; j < kRun; ++j) o[j] = f32_to_bf16_rne(f[j]);
        if (n == kRun && (((uint64_t)d) & 3) == 0) {
          uint32_t p[8];
#pragma unroll
          for (int q = 0; q < 8; ++q)
            p[q] = (uint32_t)o[q * 2] | ((uint32_t)o[q * 2 + 1] << 16);
          if ((((uint64_t)d) & 15) == 0) {
            ((uint4*)d)[0] = make_uint4(p[0], p[1], p[2], p[3]);
            ((uint4*)d)[1] = make_uint4(p[4], p[5], p[6], p[7]);
          } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) ((uint32_t*)d)[q] = p[q];
          }
        } else {
#pragma unroll
          for (int j = 0; j < kRun; ++j)
            if (j < n) d[j] = o[j];
        }
      }
    }
  }
}

// i / block == i >> shift for every i < dim: a power-of-two block, or a
// block that covers the whole dimension (quotient 0).  -1: divide.
int block_shift(int64_t block, int64_t dim) {
  if (block >= dim) return 63;
  if ((block & (block - 1)) == 0) return __builtin_ctzll((uint64_t)block);
  return -1;
}

}  // namespace

// What one pass of the largest grid covers, before its stride loops turn:
// [0] elements in all, [1] columns of one row.  Tests size their
// grid-stride cases from these.
extern "C" void fp8_block_dequant_pass_limits(int64_t* out) {
  out[0] = (int64_t)kMaxBlocks * kLanesX * kRowsPerBlock * kRun;
  out[1] = (int64_t)kMaxGridX * kLanesX * kRun;
}

extern "C" void launch_fp8_block_dequant(
    const void* src_fp8, const void* scale, int scale_dtype /*0=f32 1=bf16 2=f16*/,
    void* dst, int dst_dtype /*0=bf16 1=f32*/,
    int64_t rows, int64_t cols, int64_t block_rows, int64_t block_cols,
    hipStream_t stream) {
  if (rows <= 0 || cols <= 0 || block_rows <= 0 || block_cols <= 0) return;
  uint64_t runs_per_row = ((uint64_t)cols + kRun - 1) / kRun;
  uint64_t scale_cols = ((uint64_t)cols + block_cols - 1) / block_cols;
  uint64_t want_x = (runs_per_row + kLanesX - 1) / kLanesX;
  uint64_t want_y = ((uint64_t)rows + kRowsPerBlock - 1) / kRowsPerBlock;
  unsigned gx = want_x > (uint64_t)kMaxGridX ? kMaxGridX : (unsigned)want_x;
  uint64_t cap_y = kMaxBlocks / gx;
  unsigned gy = want_y > cap_y ? (unsigned)cap_y : (unsigned)want_y;
  dim3 grid(gx, gy), block(kLanesX, kRowsPerBlock);
  int row_shift = block_shift(block_rows, rows);
  int col_shift = block_shift(block_cols, cols);
  if (dst_dtype == 1) {
    hipLaunchKernelGGL(fp8_block_dequant_kernel<true>, grid, block, 0, stream,
                       (const uint8_t*)src_fp8, (const uint8_t*)scale,
                       scale_dtype, dst, (uint64_t)rows, (uint64_t)cols,
                       (uint64_t)block_rows, (uint64_t)block_cols, row_shift,
                       col_shift, scale_cols, runs_per_row);
  } else {
    hipLaunchKernelGGL(fp8_block_dequant_kernel<false>, grid, block, 0,
                       stream, (const uint8_t*)src_fp8,
                       (const uint8_t*)scale, scale_dtype, dst,
                       (uint64_t)rows, (uint64_t)cols, (uint64_t)block_rows,
                       (uint64_t)block_cols, row_shift, col_shift, scale_cols,
                       runs_per_row);
  }
}
