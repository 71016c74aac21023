// CDNA4 parquet page decoder: decompressed data pages -> typed,
// entry-aligned column buffers.  One wave per page.
//
// A data page (after decompression) is
//   [repetition levels][definition levels][values]
// v1: each level stream present (max level > 0) is prefixed by a u32 LE
//     byte length; v2: the two lengths come from the page header and the
//     streams carry no prefix.
// Levels and dictionary indices use parquet's RLE/bit-packed hybrid:
//   run header = ULEB128 varint h
//     h & 1 == 0: RLE run of h >> 1 copies of one value stored in
//                 ceil(bw / 8) bytes, little endian
//     h & 1 == 1: bit-packed run of (h >> 1) groups of 8 values, bw bits
//                 each, LSB first; the last group of a stream may be
//                 padded past num_values
// Values are PLAIN (fixed 4 or 8 bytes, one per entry whose definition
// level equals max_def) or a one-byte bit width followed by a hybrid
// stream of indices into the chunk's PLAIN dictionary page.
//
// Output is aligned to level ENTRIES: slot i of the value buffer belongs to
// level entry i and is zero when that entry carries no value.
//
// Execution shape shared with snappy.hip / lz4.hip: all 64 lanes parse run
// headers REDUNDANTLY in lockstep (uniform control flow, every error is a
// wave-uniform value), and expand each run cooperatively — an RLE run is a
// broadcast fill, in a bit-packed run lane j extracts value j at bit j*bw.
// The "k-th value -> entry" mapping is a ballot/popcount prefix over 64
// entries at a time.  Dictionary indices pass through a dense u32 scratch
// sized by the host from num_values.
//
// Every read is bounded by the page length / dictionary count and every
// write by num_values; a malformed page ends with a negative status.

#include <hip/hip_runtime.h>

namespace {

enum {
  PQ_OK = 0,
  PQ_ERR_FORMAT = -2,    // bit width > 32, run header varint too long
  PQ_ERR_OVERRUN = -3,   // a run claims more values than num_values
  PQ_ERR_UNDERRUN = -4,  // stream or values region ends early
  PQ_ERR_LEVEL_LEN = -5, // level stream length exceeds the page
  PQ_ERR_DICT_INDEX = -6,// dictionary index >= dictionary count
  PQ_ERR_LEVEL = -7,     // level above the column's maximum
};

struct __align__(16) PqDesc {
  uint64_t src;         // decompressed page
  uint64_t src_len;
  uint64_t dict;        // PLAIN dictionary values (0: none)
  uint64_t dict_count;
  uint64_t out_vals;    // num_values elements of `width` bytes
  uint64_t out_def;     // num_values u8 (unused when max_def == 0)
  uint64_t out_rep;     // num_values u8 (unused when max_rep == 0)
  uint64_t scratch;     // num_values u32 (dictionary pages only)
  uint64_t num_values;
  // width | dict_encoded << 8 | v2 << 16 | max_def << 24 | max_rep << 32
  uint64_t params;
  uint64_t rep_len;     // v2 only
  uint64_t def_len;     // v2 only
  int64_t status;       // out
  uint64_t non_null;    // out: entries whose level == max_def
  uint64_t consumed;    // out: offset of the values region
  uint64_t _pad;
};

__device__ inline int bits_for(uint32_t max_level) {
  return max_level ? 32 - __clz(max_level) : 0;
}

// Decode `count` values of a hybrid stream p[0, len) into out[0, count).
// Values must be < limit (err_limit otherwise).  *n_match counts values
// equal to `match`.  Returns a wave-uniform status.
template <typename T>
__device__ int hybrid_decode(const uint8_t* __restrict__ p, uint64_t len,
                             int bw, uint64_t count, T* __restrict__ out,
                             uint64_t limit, int err_limit, uint32_t match,
                             uint64_t* n_match, int lane) {
  if (bw < 0 || bw > 32) return PQ_ERR_FORMAT;
  const uint64_t vmask = bw == 32 ? 0xFFFFFFFFull : ((1ull << bw) - 1);
  const int vbytes = (bw + 7) >> 3;
  uint64_t pos = 0;
  uint64_t done = 0;
  uint64_t matched = 0;
  while (done < count) {
    // ---- run header (varint, at most 5 bytes for a 32-bit count) -------
    uint64_t h = 0;
    int shift = 0;
    while (true) {
      if (pos >= len) return PQ_ERR_UNDERRUN;
      if (shift > 28) return PQ_ERR_FORMAT;
      uint8_t b = p[pos++];
      h |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) break;
      shift += 7;
    }
    const uint64_t left = count - done;
    if (!(h & 1)) {
      // ---- RLE run: broadcast fill -----------------------------------
      uint64_t run = h >> 1;
      if (run > left) return PQ_ERR_OVERRUN;
      if (pos + vbytes > len) return PQ_ERR_UNDERRUN;
      uint64_t v = 0;
      for (int k = 0; k < vbytes; ++k) v |= (uint64_t)p[pos + k] << (8 * k);
      pos += vbytes;
      v &= vmask;
      if (run && v >= limit) return err_limit;
      for (uint64_t k = lane; k < run; k += 64) out[done + k] = (T)v;
      if ((uint32_t)v == match) matched += run;
      done += run;
    } else {
      // ---- bit-packed run: lane j extracts value j ---------------------
      uint64_t groups = h >> 1;
      uint64_t nvals = groups * 8;
      // only the final group's padding may pass num_values
      if (nvals > left && nvals - left >= 8) return PQ_ERR_OVERRUN;
      uint64_t take = nvals < left ? nvals : left;
      uint64_t need = (take * (uint64_t)bw + 7) >> 3;
      if (need > len - pos) return PQ_ERR_UNDERRUN;
      const uint64_t end = pos + need;
      for (uint64_t base = 0; base < take; base += 64) {
        uint64_t i = base + lane;
        bool live = i < take;
        uint64_t v = 0;
        if (live) {
          uint64_t bit = i * (uint64_t)bw;
          uint64_t at = pos + (bit >> 3);
          uint64_t w = 0;
          for (int k = 0; k < 5; ++k)
            if (at + k < end) w |= (uint64_t)p[at + k] << (8 * k);
          v = (w >> (bit & 7)) & vmask;
          out[done + i] = (T)v;
        }
        if (__ballot(live && v >= limit) != 0) return err_limit;
        matched += __popcll(__ballot(live && (uint32_t)v == match));
      }
      pos += groups * (uint64_t)bw;  // past len only when done == count
      done += take;
    }
  }
  *n_match = matched;
  return PQ_OK;
}

template <typename V>
__device__ inline V load_unaligned(const uint8_t* p) {
  V v;
  __builtin_memcpy(&v, p, sizeof(V));
  return v;
}

// Place the dense value stream at the entries whose level == max_def.
template <typename V>
__device__ void expand(const PqDesc* d, const uint8_t* vals, bool dict_enc,
                       uint32_t max_def, uint64_t n, int lane) {
  V* out = (V*)d->out_vals;
  const uint8_t* def = (const uint8_t*)d->out_def;
  const uint32_t* idx = (const uint32_t*)d->scratch;
  const uint8_t* dict = (const uint8_t*)d->dict;
  uint64_t k0 = 0;  // values consumed before this group of 64 entries
  for (uint64_t e0 = 0; e0 < n; e0 += 64) {
    uint64_t e = e0 + lane;
    bool live = e < n;
    bool has = live && (max_def == 0 || def[e] == max_def);
    unsigned long long m = __ballot(has);
    uint64_t k = k0 + __popcll(m & ((1ull << lane) - 1));
    V v = 0;
    if (has) {
      // k < non_null, idx[k] < dict_count: both checked by the caller
      v = dict_enc ? load_unaligned<V>(dict + (uint64_t)idx[k] * sizeof(V))
                   : load_unaligned<V>(vals + k * sizeof(V));
    }
    if (live) out[e] = v;
    k0 += __popcll(m);
  }
}

__device__ int decode_page(PqDesc* d, int lane, uint64_t* non_null_out,
                           uint64_t* consumed_out) {
  const uint8_t* src = (const uint8_t*)d->src;
  const uint64_t slen = d->src_len;
  const uint64_t n = d->num_values;
  const uint64_t params = d->params;
  const int width = (int)(params & 0xFF);
  const bool dict_enc = ((params >> 8) & 0xFF) != 0;
  const bool v2 = ((params >> 16) & 0xFF) != 0;
  const uint32_t max_def = (uint32_t)((params >> 24) & 0xFF);
  const uint32_t max_rep = (uint32_t)((params >> 32) & 0xFF);
  if (width != 4 && width != 8) return PQ_ERR_FORMAT;

  // ---- locate the level streams ----------------------------------------
  uint64_t pos = 0;
  uint64_t rep_at = 0, rep_n = 0, def_at = 0, def_n = 0;
  if (v2) {
    if (d->rep_len > slen || d->def_len > slen - d->rep_len)
      return PQ_ERR_LEVEL_LEN;
    rep_at = 0;
    rep_n = d->rep_len;
    def_at = rep_n;
    def_n = d->def_len;
    pos = rep_n + def_n;
  } else {
    if (max_rep) {
      if (slen - pos < 4) return PQ_ERR_LEVEL_LEN;
      rep_n = load_unaligned<uint32_t>(src + pos);
      pos += 4;
      if (rep_n > slen - pos) return PQ_ERR_LEVEL_LEN;
      rep_at = pos;
      pos += rep_n;
    }
    if (max_def) {
      if (slen - pos < 4) return PQ_ERR_LEVEL_LEN;
      def_n = load_unaligned<uint32_t>(src + pos);
      pos += 4;
      if (def_n > slen - pos) return PQ_ERR_LEVEL_LEN;
      def_at = pos;
      pos += def_n;
    }
  }
  *consumed_out = pos;

  // ---- levels -----------------------------------------------------------
  uint64_t unused = 0;
  uint64_t non_null = n;
  int err;
  if (max_rep) {
    err = hybrid_decode<uint8_t>(src + rep_at, rep_n, bits_for(max_rep), n,
                                 (uint8_t*)d->out_rep,
                                 (uint64_t)max_rep + 1, PQ_ERR_LEVEL,
                                 0xFFFFFFFFu, &unused, lane);
    if (err) return err;
  }
  if (max_def) {
    err = hybrid_decode<uint8_t>(src + def_at, def_n, bits_for(max_def), n,
                                 (uint8_t*)d->out_def,
                                 (uint64_t)max_def + 1, PQ_ERR_LEVEL,
                                 max_def, &non_null, lane);
    if (err) return err;
  }
  *non_null_out = non_null;

  // ---- values -----------------------------------------------------------
  const uint8_t* vals = src + pos;
  const uint64_t vlen = slen - pos;
  if (dict_enc) {
    if (non_null) {
      if (vlen < 1) return PQ_ERR_UNDERRUN;
      int bw = vals[0];
      err = hybrid_decode<uint32_t>(vals + 1, vlen - 1, bw, non_null,
                                    (uint32_t*)d->scratch, d->dict_count,
                                    PQ_ERR_DICT_INDEX, 0xFFFFFFFFu, &unused,
                                    lane);
      if (err) return err;
    }
  } else {
    if (non_null > vlen / (uint64_t)width) return PQ_ERR_UNDERRUN;
  }

  // the expansion reads back levels and indices other lanes stored
  __syncthreads();
  if (width == 4)
    expand<uint32_t>(d, vals, dict_enc, max_def, n, lane);
  else
    expand<uint64_t>(d, vals, dict_enc, max_def, n, lane);
  return PQ_OK;
}

__global__ void __launch_bounds__(64)
parquet_decode_kernel(PqDesc* __restrict__ descs, int n_pages) {
  int lane = threadIdx.x;
  for (int pidx = blockIdx.x; pidx < n_pages; pidx += gridDim.x) {
    PqDesc* d = &descs[pidx];
    uint64_t non_null = 0;
    uint64_t consumed = 0;
    // every lane holds the same decode state, so err is wave-uniform and
    // the barriers inside decode_page are reached by all lanes or none
    int err = decode_page(d, lane, &non_null, &consumed);
    if (lane == 0) {
      d->status = err;
      d->non_null = non_null;
      d->consumed = consumed;
    }
    __syncthreads();
  }
}

// One bare hybrid stream -> u32 values: the decode of levels and
// dictionary indices on its own, at any bit width 0..32.
struct __align__(16) HybridDesc {
  uint64_t src;
  uint64_t src_len;
  uint64_t dst;       // count u32
  uint64_t count;
  uint64_t bw;
  uint64_t limit;     // values must be < limit (0: no limit)
  int64_t status;     // out
  uint64_t matched;   // out: values equal to limit - 1
};

__global__ void __launch_bounds__(64)
parquet_hybrid_kernel(HybridDesc* __restrict__ descs, int n_streams) {
  int lane = threadIdx.x;
  for (int sidx = blockIdx.x; sidx < n_streams; sidx += gridDim.x) {
    HybridDesc* d = &descs[sidx];
    uint64_t matched = 0;
    uint64_t limit = d->limit ? d->limit : (1ull << 32);
    int bw = d->bw > 32 ? 33 : (int)d->bw;
    int err = hybrid_decode<uint32_t>(
        (const uint8_t*)d->src, d->src_len, bw, d->count,
        (uint32_t*)d->dst, limit, PQ_ERR_DICT_INDEX,
        (uint32_t)(limit - 1), &matched, lane);
    if (lane == 0) {
      d->status = err;
      d->matched = matched;
    }
    __syncthreads();
  }
}

inline int grid_for(int n, int max_blocks) {
  int cap = max_blocks > 0 && max_blocks < 4096 ? max_blocks : 4096;
  return n < cap ? n : cap;
}

}  // namespace

extern "C" void launch_parquet_decode(const uint64_t* desc, int n_pages,
                                      hipStream_t stream, int max_blocks) {
  if (n_pages <= 0) return;
  hipLaunchKernelGGL(parquet_decode_kernel,
                     dim3(grid_for(n_pages, max_blocks)), dim3(64), 0,
                     stream, (PqDesc*)desc, n_pages);
}

extern "C" void launch_parquet_hybrid(const uint64_t* desc, int n_streams,
                                      hipStream_t stream, int max_blocks) {
  if (n_streams <= 0) return;
  hipLaunchKernelGGL(parquet_hybrid_kernel,
                     dim3(grid_for(n_streams, max_blocks)), dim3(64), 0,
                     stream, (HybridDesc*)desc, n_streams);
}
