// What the byte-LZ stream kernels (snappy.hip, lz4.hip, inflate.hip)
// share: the stream descriptor, the status codes, the wave-cooperative
// copies through the LDS output window, and the launch rule.  Device
// code plus one host-side launcher; format parsing stays in the kernels.
//
// Execution shape: one wave per stream, all 64 lanes hold the same
// decode state (redundant lockstep), and the wave executes each literal
// run / match copy cooperatively.  Every output byte is written to HBM
// (fire-and-forget) AND to win[pos & (WIN-1)], so window slot
// p & (WIN-1) is valid for p in [op-WIN, op).
//
// L is the length/index type of the copy loops: uint64_t for snappy and
// lz4, uint32_t for inflate (whose lengths are <= 65535); positions in
// the output are uint64_t everywhere.
#pragma once

#include <hip/hip_runtime.h>

namespace lzw {

enum {
  LZ_OK = 0,
  LZ_ERR_FORMAT = -2,
  LZ_ERR_OVERFLOW = -3,
  LZ_ERR_UNDERRUN = -4,
};

// 8 u64 per stream, packed by engine/formats/compress.py
struct __align__(16) StreamDesc {
  uint64_t src;
  uint64_t src_len;
  uint64_t dst;
  uint64_t dst_cap;
  uint64_t written;   // out
  int64_t status;     // out
  uint64_t consumed;  // out
  uint64_t _pad1;     // zstd keeps its workspace pointer here
};

// Literal run: len bytes from src to out[op..] and the window.
template <int WIN, typename L>
__device__ __forceinline__ void put_run(uint8_t* out, uint8_t* win,
                                        uint64_t op, const uint8_t* src,
                                        L len, int lane) {
  for (L k = lane; k < len; k += 64) {
    uint8_t v = src[k];
    out[op + k] = v;
    win[(op + k) & (WIN - 1)] = v;
  }
}

// Drain this wave's LDS traffic (window) or its HBM traffic (out).
template <bool HBM>
__device__ __forceinline__ void drain() {
  if constexpr (HBM)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// len bytes from dist back, read from the window (HBM=false) or from
// out itself (HBM=true).  The reads need every earlier write of their
// source to have landed, hence the drain up front.  An overlapping
// match (dist < len) reads what it has just written, so it goes in
// dist-sized chunks with a drain after each.
template <int WIN, bool HBM, typename L>
__device__ __forceinline__ void copy_back(uint8_t* out, uint8_t* win,
                                          uint64_t op, L dist, L len,
                                          int lane) {
  drain<HBM>();
  if (dist >= len) {
    for (L k = lane; k < len; k += 64) {
      uint8_t v = HBM ? out[op + k - dist]
                      : win[(op + k - dist) & (WIN - 1)];
      out[op + k] = v;
      win[(op + k) & (WIN - 1)] = v;
    }
  } else {
    L copied = 0;
    while (copied < len) {
      L n = dist < len - copied ? dist : len - copied;
      for (L k = lane; k < n; k += 64) {
        uint8_t v = HBM ? out[op + copied + k - dist]
                        : win[(op + copied + k - dist) & (WIN - 1)];
        out[op + copied + k] = v;
        win[(op + copied + k) & (WIN - 1)] = v;
      }
      drain<HBM>();
      copied += n;
    }
  }
}

// Match copy: len bytes from dist bytes back (1 <= dist <= op, checked
// by the caller) to out[op..] and the window.  The LDS path needs only
// dist <= WIN; the 128 bytes are margin for the same-iteration write
// ordering.  A farther match reads old output from HBM behind a drain
// of our own stores.  FAR=false compiles that branch out for a format
// whose distance cannot exceed WIN.
template <int WIN, bool FAR, typename L>
__device__ __forceinline__ void copy_match(uint8_t* out, uint8_t* win,
                                           uint64_t op, L dist, L len,
                                           int lane) {
  if (!FAR || dist <= (L)(WIN - 128))
    copy_back<WIN, false>(out, win, op, dist, len, lane);
  else
    copy_back<WIN, true>(out, win, op, dist, len, lane);
}

// One wave per stream; a block walks the streams in strides of the grid.
inline void launch_streams(void (*kernel)(StreamDesc*, int),
                           const uint64_t* desc, int n_streams,
                           hipStream_t stream) {
  if (n_streams <= 0) return;
  int blocks = n_streams < 4096 ? n_streams : 4096;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), 0, stream,
                     (StreamDesc*)desc, n_streams);
}

}  // namespace lzw
